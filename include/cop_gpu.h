/*
 * cop_gpu.h — C-ABI boundary of the MI355X coprocessor NF pipeline.
 *
 * This is the drop-in boundary for the per-packet coprocessor path of
 * google/ghost-dataplane (reference, read-only at /root/reference):
 *
 *   engine/switch.c:443-474   coprocessor()        burst loop, forward/free
 *   engine/coprocessor.c:21-65 coprocessor_setup / coprocessor_teardown /
 *                              process_packet       (declared coprocessor.h:23-30)
 *   engine/nfs/firewall/firewall.c:170-213 fw_packet_handler
 *   engine/nfs/firewall/firewall.c:215-255 lpm_setup (rte_lpm_create/add)
 *   engine/nfs/firewall/firewall.c:276-323 setup_rules (rules.json loader)
 *   engine/switch.c:93-136    get_next_hop (parse + vport route)
 *   engine/init.c:40-84       read_config (routing table defaults)
 *
 * Everything here is plain C: pointers, sizes, negative-errno return codes.
 * No torch, no CUDA-compat headers; HIP is called only inside libcopgpu.so.
 */
#ifndef COP_GPU_H
#define COP_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Constants mirrored from the reference                                    */
/* ------------------------------------------------------------------------ */

#define COP_UNKNOWN_PORT      0xFFFFu   /* UNKNOWN_PORT       init.h:28 */
#define COP_ROUTING_TBL_SZ    0x10000u  /* ROUTING_TBL_SZ     init.h:29 */
#define COP_PKT_BURST_SZ      32u       /* PKT_BURST_SZ       init.h:47 */
#define COP_KNI_KTHREAD       5u        /* KNI_KTHREAD        init.h:52 */
#define COP_NF_QUEUE_RINGSIZE 16384u    /* NF_QUEUE_RINGSIZE  init.h:54 */
#define COP_ETHER_TYPE_IPV4   0x0800u   /* ETHER_TYPE_IPv4    switch.c:118 */
#define COP_FW_MAX_RULES      1024u     /* conf.max_rules     firewall.c:234 */
#define COP_FW_NUMBER_TBL8S   24u       /* conf.number_tbl8s  firewall.c:235 */
#define COP_LPM_MAX_DEPTH     32u       /* RTE_LPM_MAX_DEPTH  (DPDK rte_lpm.h) */
#define COP_LPM_NH_MASK       0x00FFFFFFu /* 24-bit next hop  (DPDK v1604 ABI) */

/* Stage flags. The reference selects stages at compile time with
 * ENABLE_FW_NF / DISABLE_NF (coprocessor.h:19-21, switch.c:411,426,524);
 * the same macro names select COP_DEFAULT_STAGES here, and cop_config.stages
 * carries the mask to the device at run time. */
#define COP_STAGE_PARSE 0x1u  /* get_next_hop switch.c:93-136            */
#define COP_STAGE_FW    0x2u  /* fw_packet_handler firewall.c:170-213    */
#define COP_STAGE_LPM   0x4u  /* route LPM on dst (north-star extension) */

#if defined(DISABLE_NF)
#define COP_DEFAULT_STAGES (COP_STAGE_PARSE)
#elif defined(ENABLE_FW_NF)
#define COP_DEFAULT_STAGES (COP_STAGE_PARSE | COP_STAGE_FW)
#else
#define COP_DEFAULT_STAGES (COP_STAGE_PARSE | COP_STAGE_FW)
#endif

/* Stages of the drop-in coprocessor API (process_packet, process_burst,
 * cop_coprocessor_poll*): the coprocessor thread's NF chain only. Parse and
 * vport routing (get_next_hop, the UNKNOWN_PORT drop) are the fast path's
 * job before a packet is enqueued to the coprocessor (switch.c:406-415), so
 * the drop-in never drops on them: an IPv4 packet whose dst&0xFFFF is in
 * 0..4, or an IPv6 EtherType, gets the firewall's verdict. The batch API
 * (cop_submit*, cop_process_host*) runs cop_config.stages.
 *   - process_packet runs fw_packet_handler under ENABLE_FW_NF
 *     (coprocessor.c:59-62), which the reference's coprocessor.h:21 always
 *     defines: COP_STAGE_FW, also when neither macro is defined.
 *   - DISABLE_NF (coprocessor.h:19): switch.c never calls the coprocessor
 *     (switch.c:411,426,524); if it is called anyway, every packet forwards
 *     (no NF stage), as process_packet does without ENABLE_FW_NF
 *     (coprocessor.c:59-64). Define COP_DROPIN_NO_NF for that chain alone.
 * The library is built once, so the caller's macros reach it through
 * coprocessor_setup, which this header makes an alias of
 * cop_coprocessor_setup_fw or cop_coprocessor_setup_no_nf in the caller's
 * build (cop_set_dropin_stages sets the same at run time, e.g. from an FFI). */
#if defined(DISABLE_NF) || defined(COP_DROPIN_NO_NF)
#define COP_DROPIN_STAGES 0u
#else
#define COP_DROPIN_STAGES (COP_STAGE_FW)
#endif

/* Per-packet verdicts (one byte of the result record).
 *   FORWARD/DROP_FW : enum FW_ACTION firewall.h:71-74 (FW_FORWARD=0, FW_DROP=1)
 *   DROP_PARSE      : get_next_hop() == UNKNOWN_PORT, freed by the fast path
 *                     (switch.c:406-410); never reaches the coprocessor
 *   DROP_NOT_IPV4   : version nibble != 4. The reference counts it
 *                     (firewall.c:186-190) and then dereferences NULL at
 *                     firewall.c:193-194 (undefined behaviour); this build
 *                     defines the outcome as a drop.
 *   DROP_NO_PORT    : port >= number of active vports; the reference's
 *                     enqueue_nf_rx silently discards it (switch.c:316-319). */
enum cop_verdict {
    COP_FORWARD       = 0,
    COP_DROP_FW       = 1,
    COP_DROP_PARSE    = 2,
    COP_DROP_NOT_IPV4 = 3,
    COP_DROP_NO_PORT  = 4
};

#define COP_FLAG_ROUTE_HIT 0x1u /* route LPM lookup hit (rte_lpm_lookup ret == 0) */
#define COP_FLAG_FW_HIT    0x2u /* firewall LPM lookup hit                         */

/* 8-byte per-packet result record (SURVEY.md §8a "bit-exact contract"). */
typedef struct cop_result {
    uint8_t  verdict;   /* enum cop_verdict */
    uint8_t  flags;     /* COP_FLAG_* */
    uint16_t port;      /* vport from the routing table, or COP_UNKNOWN_PORT */
    uint32_t route_nh;  /* 24-bit next hop of the route LPM stage (0 on miss) */
} cop_result;

/* One prefix rule: struct fw_rule firewall.h:49-53 ({src_ip, depth, action})
 * generalised to a 24-bit next hop so the same type carries route prefixes. */
typedef struct cop_prefix {
    uint32_t ip;        /* host byte order, unmasked (rte_lpm_add masks it) */
    uint32_t next_hop;  /* FW: action (uint8 in the reference); routes: 24-bit */
    uint8_t  depth;     /* 1..32 accepted; anything else is -EINVAL */
    uint8_t  _pad[3];
} cop_prefix;

/* rte_lpm_config as used by lpm_setup (firewall.c:229-235). */
typedef struct cop_lpm_config {
    uint32_t max_rules;     /* distinct (prefix, depth) rules; default 1024 */
    uint32_t number_tbl8s;  /* tbl8 groups (/24s holding a depth>24 prefix); default 24 */
    uint32_t flags;         /* COP_LPM_* */
} cop_lpm_config;

/* Reproduce lpm_setup's "print, return 1 at the first failed rte_lpm_add"
 * (firewall.c:245-251): every later rule is dropped. Without this flag a
 * failed rule is skipped, counted in the report, and loading continues. */
#define COP_LPM_STOP_AT_FIRST_ERROR 0x1u

typedef struct cop_lpm_report {
    uint32_t n_in;            /* rules presented */
    uint32_t n_added;         /* rte_lpm_add calls that returned 0 */
    uint32_t n_distinct;      /* distinct rules held (rule-table occupancy) */
    uint32_t n_updated;       /* adds that hit an existing rule (last write wins) */
    uint32_t n_failed;        /* adds that returned < 0 */
    uint32_t n_skipped;       /* rules never presented (after a stop-at-first-error) */
    int32_t  first_error;     /* errno of the first failure (negative) or 0 */
    uint32_t first_error_idx; /* index of the first failed rule */
    uint32_t tbl8_used;       /* tbl8 groups in use */
    uint32_t n_intervals;     /* disjoint address intervals of the flattened table */
} cop_lpm_report;

/* ------------------------------------------------------------------------ */
/* Host-side LPM table (build once, upload to every GPU context)            */
/* ------------------------------------------------------------------------ */

typedef struct cop_lpm_table cop_lpm_table;

/* Build a table with DPDK rte_lpm_add semantics:
 * depth 1..32 else -EINVAL; ip masked to depth; a duplicate (prefix, depth)
 * overwrites the next hop; a new rule fails -ENOSPC once max_rules distinct
 * rules are held, or when it needs a tbl8 group and all number_tbl8s are in
 * use; a failed add leaves the table unchanged. Returns 0 or -errno. */
int  cop_lpm_build(const cop_prefix *rules, uint32_t n, const cop_lpm_config *cfg,
                   cop_lpm_table **out, cop_lpm_report *report);
void cop_lpm_free(cop_lpm_table *t);
/* Export the DIR-24-8 image: tbl24 has 1<<24 entries, tbl8 has tbl8_used*256.
 * Entry layout: bits 0-23 next hop (or tbl8 group), bit 24 valid,
 * bit 25 valid_group (extended), bits 26-31 depth — the DPDK v1604 layout. */
int  cop_lpm_export_dir24(const cop_lpm_table *t, uint32_t *tbl24, uint32_t *tbl8,
                          uint32_t tbl8_cap_entries);
/* Export the flattened form: starts[k] ascending, starts[0] == 0; value[k] =
 * (hit << 24) | next_hop for addresses in [starts[k], starts[k+1]). */
int  cop_lpm_export_intervals(const cop_lpm_table *t, uint32_t *starts, uint32_t *values,
                              uint32_t cap);
/* Accepted rule set after all adds: masked prefix, depth, final next hop.
 * The position in this list is the rule id (first-acceptance order of the
 * distinct (prefix, depth) pairs); per-rule hit counters are indexed by it. */
int  cop_lpm_export_rules(const cop_lpm_table *t, cop_prefix *out, uint32_t cap);
/* Host lookup of the matching (longest-prefix) rule id per address, -1 on a
 * miss. Setup/diagnostic use; the data path runs on the GPU. */
int  cop_lpm_lookup_rules(const cop_lpm_table *t, const uint32_t *ips, uint32_t n, int32_t *rule_id);

/* Live tables: every table, built or created empty, can be changed one rule
 * at a time (rte_lpm_add / rte_lpm_delete / rte_lpm_delete_all /
 * rte_lpm_is_rule_present). After each successful
 * call the lookups, the exports above and the report equal those of a table
 * built from the rules now held; the work is proportional to the changed
 * prefix's subtree. A table is not thread-safe: one writer at a time, and
 * no reader during a write.
 *   cop_lpm_create    an empty table; cfg NULL = 1024 rules / 24 groups.
 *   cop_lpm_add       cop_lpm_build's acceptance rules for one rule: -EINVAL
 *                     (depth outside 1..32), -ENOSPC (max_rules held, or a
 *                     depth > 24 rule in a /24 without a tbl8 group when all
 *                     number_tbl8s are in use), 0 (added, or the next hop of
 *                     a held (prefix, depth) overwritten).
 *   cop_lpm_delete    -EINVAL for a bad depth and for a rule that is not
 *                     held (DPDK's value, not -ENOENT); else the rule leaves
 *                     and its addresses fall back to the longest remaining
 *                     covering rule or to a miss. A /24's tbl8 group is in
 *                     use while the /24 holds a rule deeper than 24; deleting
 *                     the last one releases it (tbl8_recycle_check).
 *   cop_lpm_is_rule_present  1 (and *next_hop, if not NULL), 0, or -EINVAL.
 * A failed call leaves the table unchanged. Rule ids: a delete frees its id
 * and moves no other; a new rule takes the lowest free id, so a table never
 * deleted from keeps first-acceptance order. cop_lpm_export_rules skips
 * freed ids; cop_lpm_export_rules_ids also returns each rule's id (out / ids
 * NULL: the count; -ENOSPC if more than cap). cop_lpm_generation counts the
 * successful mutations since the table was made. */
int  cop_lpm_create(const cop_lpm_config *cfg, cop_lpm_table **out);
int  cop_lpm_add(cop_lpm_table *t, uint32_t ip, uint8_t depth, uint32_t next_hop);
int  cop_lpm_delete(cop_lpm_table *t, uint32_t ip, uint8_t depth);
int  cop_lpm_delete_all(cop_lpm_table *t);
int  cop_lpm_is_rule_present(const cop_lpm_table *t, uint32_t ip, uint8_t depth, uint32_t *next_hop);
uint64_t cop_lpm_generation(const cop_lpm_table *t);
int  cop_lpm_export_rules_ids(const cop_lpm_table *t, cop_prefix *out, uint32_t *ids, uint32_t cap);

/* ------------------------------------------------------------------------ */
/* Rule files (rules.json format, firewall.c:57-105,276-323)                */
/* ------------------------------------------------------------------------ */

/* Parse a rules file: a JSON object (or array) whose children are objects
 * with case-insensitive keys "ip" (dotted quad, parsed with the reference's
 * sscanf("%u.%u.%u.%u") and &0xff per byte), "depth" and "action" (cJSON
 * valueint truncated to uint8). *out is malloc'd; free with cop_rules_free.
 * Errors: -ENOENT (open), -EINVAL (syntax, missing key, bad ip). */
int  cop_rules_load_json(const char *path, cop_prefix **out, uint32_t *n);
void cop_rules_free(cop_prefix *rules);
/* Write rules pretty-printed with short lines (<255 chars, firewall.c:72,95). */
int  cop_rules_write_json(const char *path, const cop_prefix *rules, uint32_t n);
/* Binary prefix dump for large sets: 16-byte header ("CPRB", u32 version 1,
 * u64 count) + count 12-byte cop_prefix records, little-endian, file order.
 * load: *out malloc'd (free with cop_rules_free); -ENOENT (open), -EINVAL
 * (magic, version, or size != header + count * 12), -ENOMEM, -EIO. */
int  cop_rules_load_bin(const char *path, cop_prefix **out, uint32_t *n);
int  cop_rules_write_bin(const char *path, const cop_prefix *rules, uint32_t n);

/* Default vport routing table (read_config, init.c:40-84): all 0, entries
 * 0..n_ports-1 = UNKNOWN_PORT, entry (192.167.10.(i+1) & 0xFFFF) = i. */
void cop_route_table_default(uint16_t *rt /* COP_ROUTING_TBL_SZ */, uint32_t n_ports);

/* ------------------------------------------------------------------------ */
/* GPU context: one per coprocessor thread or per GPU                       */
/* ------------------------------------------------------------------------ */

typedef struct cop_ctx cop_ctx;

#define COP_CFG_FW_FORCE_DIR24  0x1u  /* FW lookups from the HBM DIR-24-8 image, not LDS */
#define COP_CFG_LPM_FORCE_DIR24 0x2u  /* route lookups from HBM even if small */
#define COP_CFG_NO_COMPACT      0x4u  /* never build the ordered forward list */
#define COP_CFG_RULE_COUNTERS   0x8u  /* per-rule firewall hit counters (u64 per rule id) */
/* Demux: one ordered forward list per vport instead of one per batch — the
 * tx_q order of each port's coprocessor (enqueue_nf_rx switch.c:306-327,
 * then coprocessor() switch.c:464-470). Port q's list is at fwd_idx + q*n
 * (n = the batch's packet count), its length at fwd_count[q]; so fwd_idx
 * holds n_ports*n entries and fwd_count n_ports (ring: fwd_slot >=
 * n_ports*n, counts at fwd_count + slot*n_ports). Needs n_ports <= 8. */
#define COP_CFG_DEMUX_PORTS     0x10u
/* Per-port coprocessor_stats (switch.h:33-38) kept on the device. */
#define COP_CFG_PORT_STATS      0x20u
/* Route tables too large for LDS: look them up in the multibit-trie form
 * (12-bit top level in LDS, popcount-compressed 6-bit nodes, a few MiB that
 * stay in L2) instead of the 64 MiB DIR-24-8 image. Results are identical. */
#define COP_CFG_LPM_TRIE        0x40u
/* Segmented forward lists: a batch's ordered forward list is kept in
 * segments of COP_SEG_PKTS consecutive packets. Segment k (packets
 * k*COP_SEG_PKTS ..) holds its forwarded packets' indices, in arrival order,
 * at fwd_idx[k*COP_SEG_PKTS ..] and their number at fwd_count[k]; so
 * fwd_count holds ceil(n / COP_SEG_PKTS) words per batch (ring: per slot, at
 * fwd_count + slot*ceil(n/COP_SEG_PKTS)), and fwd_idx must be 16-byte
 * aligned (ring: fwd_slot a multiple of 4). Walking the segments in order
 * yields exactly the dense list — the tx side drains it segment by segment,
 * as coprocessor() hands its forward buffer over per burst of PKT_BURST_SZ
 * (switch.c:464-473). No tile waits for another's count, so the kernels
 * need no cross-workgroup prefix. Not combinable with DEMUX_PORTS. */
#define COP_CFG_SEG_LISTS       0x80u
#define COP_SEG_PKTS            256u
/* Route tables too large for LDS: look them up in the bucketed interval form
 * in global memory (a few MiB that stay in L2 / the Infinity Cache): the
 * bucket of the address's top bits gives the first candidate interval, one
 * 16-byte load of two (start, value) pairs decides almost every lookup.
 * Results are identical; takes precedence over COP_CFG_LPM_TRIE. */
#define COP_CFG_LPM_BKT         0x100u
/* Firewall tables too large for LDS (config 5's 1M rules) in the same
 * bucketed interval form, keyed by rule id, instead of the DIR-24-8 image:
 * about 16 + 12 MiB per 1M rules against 64 MiB, two dependent L2 / Infinity
 * Cache reads per lookup instead of one random 64 MiB probe. Results, rule
 * ids and per-rule counters are identical. */
#define COP_CFG_FW_BKT          0x200u
/* Live tables: the stage tables of this context accept cop_update_* patches
 * (below). Their DIR-24-8 images keep the tbl8 groups in the plain form
 * ($COP_TBL8=packed is ignored) with spare groups and a free list owned by
 * the context, per-rule counters are sized to the table's max_rules, and the
 * LDS interval buffers hold any table of up to 8192 intervals. Lookups and
 * results are the same as without the flag. */
#define COP_CFG_LIVE_TABLES     0x400u
#define COP_MAX_DEMUX_PORTS     8

typedef struct cop_config {
    int      device;          /* HIP device ordinal */
    uint32_t stages;          /* COP_STAGE_* mask */
    uint32_t n_ports;         /* nb_active_kni (init.c:63), default 5 */
    uint32_t max_batch;       /* packets per batch, default 262144 */
    uint32_t max_batches;     /* batches per cop_submit, default 32 */
    uint32_t flags;           /* COP_CFG_* */
    uint32_t n_streams;       /* launch lanes (HIP streams) used round-robin, 1..4, default 2 */
    const uint16_t *routing_table; /* 65536 entries, or NULL = read_config default */
} cop_config;

void cop_config_default(cop_config *cfg);

/* Returns 0 or -ENODEV (no GPU), -EINVAL, -ENOMEM, -EIO (HIP error). */
int  cop_create(const cop_config *cfg, cop_ctx **out);
void cop_destroy(cop_ctx *ctx);
const char *cop_last_error(cop_ctx *ctx);
int  cop_device_count(void);
/* PCI bus id of a device ("dddd:bb:dd.f"), so a caller can run its
 * coprocessor threads and place their host buffers on the GPU's NUMA node
 * (as DPDK places lcores on the NIC's socket). 0, -EINVAL or -ENODEV. */
int  cop_device_pci_bus_id(int device, char *buf, int len);

/* Upload tables (synchronous). The table may be freed afterwards. */
int  cop_set_fw_table(cop_ctx *ctx, const cop_lpm_table *t);
int  cop_set_route_lpm(cop_ctx *ctx, const cop_lpm_table *t);
/* The vport routing table (65536 entries, port of dst & 0xFFFF; copied). May
 * be called again at any time after cop_create: the call waits for the
 * context's launches in flight, which finish with the table they were
 * submitted under, and every later launch sees the new table (its LDS carve
 * follows the table's non-uniform 256-entry blocks, see cop_submit). Returns
 * -EINVAL for a NULL argument and -EBUSY while a poll-mode kernel serves the
 * context (cop_pmd_stop first; the kernel keeps the table it was started
 * with). */
int  cop_set_routing_table(cop_ctx *ctx, const uint16_t *rt /* 65536 */);
/* setup_rules + lpm_setup in one call: read a rules.json file and build the
 * firewall table with cfg (NULL = reference 1024/24, stop at first error). */
int  cop_load_fw_rules_file(cop_ctx *ctx, const char *path, const cop_lpm_config *cfg,
                            cop_lpm_report *report);

/* Rule updates without a rebuild. After cop_lpm_add / cop_lpm_delete on the
 * table that cop_set_fw_table / cop_set_route_lpm uploaded to a
 * COP_CFG_LIVE_TABLES context, cop_update_* brings the stage's device images
 * to the table's current generation: only the entries of the changed
 * prefixes' address ranges are written, by one patch kernel, from fill
 * records that go through pinned staging; a table of at most 8192 intervals
 * also gets its LDS interval image (about 70 KiB) copied afresh, and a table
 * that crosses that size changes form. With COP_CFG_RULE_COUNTERS the counter
 * word of every rule id freed since the last applied generation is zeroed in
 * the same order. The table object must stay alive between the calls (it is
 * recognised by identity) and is not changed by them.
 *
 * Ordering, one-shot launches (cop_submit, cop_submit_ring, the host paths):
 * the call is asynchronous and stream-ordered across all lanes. Batches
 * submitted before the call see the old rule set in every packet, batches
 * submitted after it returns see the new one, in whichever lanes they run;
 * no cop_sync is needed, and the call neither synchronises the device nor
 * frees device memory. The device never holds a half-applied update: the
 * patch waits for every lane's last launch, and every lane's next launch
 * waits for the patch.
 *
 * Ordering, while a poll-mode kernel serves the context: the kernel is
 * paused (it finishes every batch below its gates and leaves), the patch
 * runs on the free GPU, the kernel's table parameters are refreshed and it
 * is relaunched. Every batch is served wholly by one generation: batches
 * waited for before the call used the old table, batches posted after it
 * returns use the new one. -EBUSY, with the device tables untouched, when
 * the update would change the kernel's launch geometry (the stage's table
 * form, or the LDS bytes of its interval image), when it needs the
 * whole-table upload below, or when it is a firewall update on a
 * COP_CFG_RULE_COUNTERS context.
 *
 * Whole-table upload instead (rep->full = 1; synchronous, as cop_set_*): the
 * context is not COP_CFG_LIVE_TABLES; the stage holds another table or none;
 * the table's change journal (65536 mutations) no longer reaches back to the
 * generation the context holds; the image has run out of spare tbl8 groups;
 * or the stage's form is the trie or a bucketed one (COP_CFG_LPM_TRIE,
 * COP_CFG_LPM_BKT for the route stage, COP_CFG_FW_BKT for the firewall).
 *
 * Returns 0 or -errno (-EINVAL, -EBUSY, -ENOMEM, -EIO; after -EIO the next
 * update uploads the whole table). rep may be NULL. */
typedef struct cop_update_report {
    uint32_t full;          /* 1: fell back to a whole-table upload */
    uint32_t n_changes;     /* journal entries applied */
    uint32_t n_records;     /* patch records sent */
    uint32_t tbl24_entries; /* tbl24 entries written by the patch kernel */
    uint32_t tbl8_entries;  /* tbl8 entries written */
    uint32_t groups_taken, groups_released;
    uint64_t h2d_bytes;     /* bytes copied host to device for this update */
} cop_update_report;

int  cop_update_fw_table(cop_ctx *ctx, const cop_lpm_table *t, cop_update_report *rep);
int  cop_update_route_lpm(cop_ctx *ctx, const cop_lpm_table *t, cop_update_report *rep);
/* rules.json edited on disk: change t (the table the firewall stage holds)
 * until it holds what cop_lpm_build would accept from the file under t's own
 * limits (rules that left are deleted first, then new rules are added and
 * changed actions overwritten), then cop_update_fw_table. */
int  cop_update_fw_rules_file(cop_ctx *ctx, cop_lpm_table *t, const char *path, cop_update_report *rep);

/* A stage's whole table replaced in stream order. After the call returns the
 * stage holds table t at its current generation, whatever it held before:
 * another table, none, or the same table at any older generation (a reloaded
 * rule set, a new routing snapshot, a table whose journal no longer reaches
 * back). The table object must stay alive, as for cop_update_*, and a later
 * cop_update_* of it patches incrementally.
 *
 * Device path: a COP_CFG_LIVE_TABLES context whose stage is in the LDS
 * interval or the DIR-24-8 form (not COP_CFG_FW_BKT, COP_CFG_LPM_TRIE,
 * COP_CFG_LPM_BKT) and, for a firewall table on a COP_CFG_RULE_COUNTERS
 * context, whose per-rule counter words already cover max(rule ids of t, t's
 * max_rules). The table's sorted intervals (about a megabyte for 100k routes)
 * go through pinned staging and one kernel paints all of tbl24 and the tbl8
 * groups from them where the image lives; a table of at most 8192 intervals
 * also gets its LDS interval image copied, a larger one takes the stage to
 * the DIR-24-8 form; every per-rule counter word of a firewall stage is
 * zeroed, as cop_set_fw_table zeroes them. Ordering is that of cop_update_*:
 * batches and cop_lookup_bulk calls queued before the call see the old table
 * for every packet or address, those queued after it returns the new one, on
 * whichever lane; no cop_sync is needed. The call does not synchronise the
 * device, does not free device memory and does not wait for queued work (it
 * may wait for the copy of an earlier replacement's intervals out of pinned
 * staging). It allocates what is missing or outgrown (a first tbl24, a
 * larger tbl8, staging); an outgrown buffer, which queued work may still
 * read, is kept until the next cop_set_* or cop_destroy.
 *
 * While a poll-mode kernel serves the context: paused, painted, table
 * parameters and pointers refreshed, relaunched; every batch is served wholly
 * by one table. -EBUSY with the device untouched where cop_update_* refuses:
 * a changed launch geometry (the stage's form, the LDS bytes of its interval
 * image), a firewall table on a COP_CFG_RULE_COUNTERS context.
 *
 * Otherwise the call is cop_set_* (synchronous, rep->full = 1), or -EBUSY
 * under a poll-mode kernel.
 *
 * Report of the device path: full 0, n_changes 0, n_records the intervals
 * sent, tbl24_entries 1 << 24, tbl8_entries and groups_taken the new image's
 * groups (x 256), groups_released the groups the previous image used,
 * h2d_bytes the bytes copied. Errors as cop_update_*; after -EIO the next
 * cop_update_* uploads the whole table. */
int  cop_replace_fw_table(cop_ctx *ctx, const cop_lpm_table *t, cop_update_report *rep);
int  cop_replace_route_lpm(cop_ctx *ctx, const cop_lpm_table *t, cop_update_report *rep);

/* ------------------------------------------------------------------------ */
/* Bulk lookups (rte_lpm_lookup_bulk on the device) and table audit         */
/* ------------------------------------------------------------------------ */

/* An array of IPv4 addresses (host byte order) in, one word per address out,
 * straight from a stage's device table: no frames, no pipeline, no counters.
 * The word is the same from every device form of the table and from the host
 * reference cop_lpm_lookup_words:
 *   route stage / COP_LOOKUP_NH     hit:  next_hop | COP_LOOKUP_HIT
 *   firewall stage / COP_LOOKUP_RULE hit: rule_id | COP_LOOKUP_HIT
 *                                         | (action != 0 ? COP_LOOKUP_DROP : 0)
 *   miss: exactly 0. Every other bit is zero.
 * rule_id is the id of cop_lpm_export_rules_ids (the per-rule counter index).
 * Relation to DPDK: out[i] & 0x00FFFFFF and the COP_LOOKUP_HIT flag
 * (RTE_LPM_LOOKUP_SUCCESS) are what rte_lpm_lookup_bulk gives for a table
 * holding the same rules; DPDK's depth and valid_group bits are not
 * reproduced. */
#define COP_LOOKUP_HIT  0x01000000u   /* == RTE_LPM_LOOKUP_SUCCESS */
#define COP_LOOKUP_DROP 0x04000000u   /* firewall form: the matching rule's action is non-zero */
#define COP_LOOKUP_NH   0             /* form of the route stage's image */
#define COP_LOOKUP_RULE 1             /* form of the firewall stage's image */

/* Host reference: the exact word the device returns, from the host table as
 * it is now (after any cop_lpm_add / cop_lpm_delete). 0, -EINVAL (NULL, or a
 * form other than the two above), -ENOMEM. */
int  cop_lpm_lookup_words(const cop_lpm_table *t, int form, const uint32_t *ips, uint32_t n, uint32_t *out);

/* Device lookup. stage is exactly COP_STAGE_FW or COP_STAGE_LPM (else
 * -EINVAL); the stage need not be in cfg.stages but must hold a table
 * (-ENOENT). ips / out are device pointers (or mapped host memory), 4-byte
 * aligned (-EINVAL); when both are 16-byte aligned the kernel moves 16 bytes
 * per lane. out == ips (in place) is allowed, any other overlap is -EINVAL.
 * n == 0 returns 0 and launches nothing.
 *
 * The table form is the one a pipeline launch would use for that stage alone
 * (the LDS interval image, else trie / bucketed when built, else DIR-24-8
 * with plain or packed tbl8 groups), following the context's flags.
 *
 * Ordering: asynchronous, queued on the context's next launch lane
 * (round-robin, as cop_submit); outputs are valid after cop_sync. It is
 * ordered with cop_update_* like any launch: a lookup queued before
 * cop_update_* is called reads the old image for every address, one queued
 * after it returns reads the new one; no cop_sync is needed in between. No
 * counter is touched (cop_counters, port stats, per-rule hits).
 *
 * While a poll-mode kernel serves the context the call is synchronous: the
 * kernel is paused, the lookup runs on the free GPU, the kernel is
 * relaunched (as cop_counters_snapshot does); the outputs are valid on
 * return. */
int  cop_lookup_bulk(cop_ctx *ctx, uint32_t stage, const uint32_t *ips, uint32_t n, uint32_t *out);
/* The same over host arrays of any length: pinned staging in chunks, two
 * slots in turn; synchronous. out == ips is allowed. */
int  cop_lookup_bulk_host(cop_ctx *ctx, uint32_t stage, const uint32_t *ips, uint64_t n, uint32_t *out);

/* Does the stage's device image answer as host table t does, right now?
 * Probes: for every start s of t's intervals in the stage's form, s and
 * s - 1 (s > 0), plus 0xFFFFFFFF (at most 2m + 1 addresses: every interval
 * is probed at both ends). They go through cop_lookup_bulk_host's staging
 * and are compared with cop_lpm_lookup_words. Synchronous; waits for the
 * context's queued work first. Returns 0 with the report filled (a mismatch
 * is a finding, not an error) or cop_lookup_bulk's errors. Up to bad_cap
 * mismatching addresses, ascending, are written to bad_ips (may be NULL). */
typedef struct cop_audit_report {
    uint64_t n_probes, n_mismatch;
    uint64_t generation_table, generation_device; /* device: 0 when the stage is not live */
    uint32_t stale;          /* live stage holds another generation (or another table) than t */
    uint32_t form;           /* device form the lookups ran in (0 off,1 LDS,2 DIR-24-8,3 trie,4 bucketed) */
    uint32_t first_ip, first_device, first_host; /* first mismatch, if any */
    uint32_t n_bad;          /* entries written to bad_ips */
} cop_audit_report;
int  cop_lookup_audit(cop_ctx *ctx, uint32_t stage, const cop_lpm_table *t, cop_audit_report *rep,
                      uint32_t *bad_ips, uint32_t bad_cap);

/* Packed header records: a batch (or ring) with stride == COP_HDR16_STRIDE
 * and no offsets holds, instead of frames, one 16-byte record per packet:
 * frame bytes 12..15 (EtherType, version/IHL, TOS) followed by bytes 24..35
 * (IPv4 checksum, src, dst, UDP ports), the only bytes the pipeline reads.
 * Results are identical to the frames'. cop_pack_headers() builds them on
 * the host; the end-to-end host path moves 16 bytes per packet over PCIe
 * this way instead of a 64-byte header line. */
#define COP_HDR16_STRIDE 16u
void cop_pack_headers(const void *const *pkt_data, uint32_t n, uint8_t *out /* n * 16 bytes */);
/* Compact header records (cop_submit batches only, not rings): stride ==
 * COP_HDR12_STRIDE holds one 12-byte record per packet (pkts 4-byte
 * aligned), frame bytes 12..15 then 26..33 (src, dst): the bytes the
 * verdicts depend on, a quarter fewer
 * than a 16-byte record. Results are identical to the frames'. The
 * end-to-end host path (cop_process_host_stream) sends these. */
#define COP_HDR12_STRIDE 12u
void cop_pack_headers12(const void *const *pkt_data, uint32_t n, uint8_t *out /* n * 12 bytes */);

/* One batch of packets resident in device memory (HBM).
 * Packet i starts at  pkts + (offsets ? offsets[i] : i * stride) + data_off.
 * Every packet start must be 16-byte aligned and hold >= 48 readable bytes
 * (the fields sit at fixed offsets 12..33, as firewall.c:143-145 /
 * switch.c:125-127 read them; the streaming kernel moves whole 16-byte
 * chunks, and any Ethernet frame has >= 60). offsets[i] and data_off are
 * independent: their sum may pass 2^32 (the address is formed in 64 bits);
 * offsets[i] itself must be <= 2^32 - 64. Outputs: results[i] for every packet;
 * fwd_idx[0..*fwd_count) = indices of FORWARD packets in arrival order (the
 * order coprocessor() enqueues them to tx_q, switch.c:464-470). */
typedef struct cop_batch {
    const void     *pkts;      /* device pointer */
    const uint32_t *offsets;   /* device pointer or NULL (IMIX slab mode) */
    uint32_t        n;         /* packets */
    uint32_t        stride;    /* bytes between packet slots (no offsets) */
    uint32_t        data_off;  /* added to every packet start (mbuf headroom) */
    uint32_t        _pad;
    cop_result     *results;   /* device pointer, n records */
    uint32_t       *fwd_idx;   /* device pointer, n entries, or NULL */
    uint32_t       *fwd_count; /* device pointer, 1 entry, or NULL */
} cop_batch;

/* Enqueue nb batches (nb <= max_batches) as ONE kernel launch on the next
 * launch lane (stream) of the context, round-robin. Launches on different
 * lanes may run concurrently. Asynchronous: returns once queued; outputs are
 * valid after cop_sync.
 * LDS budget: a workgroup holds the routing table's image (1 KiB plus 512
 * bytes per non-uniform 256-entry block), the stages' interval tables (or the
 * trie's 16 KiB top level), its scratch words (more with DEMUX_PORTS /
 * PORT_STATS) and the tile's list stage (1 KiB per 256 packets of the tile),
 * plus $COP_LDS_PAD. A launch that needs more than 160 KiB looks the route
 * stage up in its DIR-24-8 image in HBM instead; if that is not enough, the
 * firewall stage too; if it still does not fit, the call returns -E2BIG
 * (cop_last_error names LDS) and nothing is launched or written. Results do
 * not depend on the form taken. cop_submit_ring and cop_pmd_start choose the
 * same way. */
int  cop_submit(cop_ctx *ctx, const cop_batch *batches, uint32_t nb);
/* A ring of equally shaped batch slots resident in device memory (a batch
 * ring buffer in HBM). Slot s: packets at pkts + s*pkts_slot_bytes (packet i
 * at + i*stride + data_off, or, when offsets != NULL, at + offsets_s[i] +
 * data_off with offsets_s = offsets + s*offsets_slot_words), records at
 * results + s*results_slot, forward list at fwd_idx + s*fwd_slot (may be
 * NULL), its length at fwd_count[s] (may be NULL). */
typedef struct cop_batch_ring {
    const void     *pkts;
    const uint32_t *offsets;
    cop_result     *results;
    uint32_t       *fwd_idx;
    uint32_t       *fwd_count;
    uint64_t        pkts_slot_bytes;
    uint64_t        offsets_slot_words;
    uint64_t        results_slot;      /* records per slot (>= n) */
    uint64_t        fwd_slot;          /* forward-list entries per slot (>= n) */
    uint32_t        n_slots;
    uint32_t        n;                 /* packets per batch */
    uint32_t        stride;
    uint32_t        data_off;
} cop_batch_ring;

#define COP_MAX_RING_BATCHES 1024u

/* Enqueue `count` (<= COP_MAX_RING_BATCHES) consecutive slots starting at
 * first_slot (wrapping at n_slots) as ONE kernel launch on the next lane.
 * Per-batch semantics are exactly those of cop_submit. */
int  cop_submit_ring(cop_ctx *ctx, const cop_batch_ring *ring, uint32_t first_slot, uint32_t count);

/* Block until everything submitted on every lane has completed. 0 or -EIO. */
int  cop_sync(cop_ctx *ctx);
/* Non-blocking: 0 when idle, -EAGAIN while work is in flight. */
int  cop_poll(cop_ctx *ctx);

/* ------------------------------------------------------------------------ */
/* Tx gather: forwarded frames packed into tx bursts on the device          */
/* ------------------------------------------------------------------------ */

/* The tx half of coprocessor() (switch.c:464-473) for batches resident in
 * device memory: the frames of a batch's forward list are copied, in list
 * order, into a contiguous tx burst, and what does not fit is counted as the
 * reference counts tx_dropped. One burst per forward list: out[0], or on a
 * COP_CFG_DEMUX_PORTS context out[q] for vport q (q < n_ports).
 *
 * Lists: the layout public submits on this context write: one dense list per
 * batch; with COP_CFG_DEMUX_PORTS one per vport at fwd_idx + q*n, its length
 * at fwd_count[q]; with COP_CFG_SEG_LISTS the concatenation of the batch's
 * COP_SEG_PKTS-packet segments in order. A list's length is clamped to what
 * the layout holds (n; a segment's packet count), an index to n - 1. A ring
 * slot is passed as a cop_batch whose pointers the caller computes.
 *
 * Per list L = (i_0, i_1, ...), packet i's source where cop_batch puts it:
 *   slot batch (offsets == NULL): ext_k = len_k = copy_bytes,
 *                                 off_k = k * slot_bytes;
 *   IMIX batch:  l = clamp(lens[i_k], 1, COP_TX_MAX_FRAME), len_k = l,
 *                ext_k = (l + 15) & ~15, off_k = the sum of the earlier ext;
 *                the caller guarantees ext_k readable bytes at the packet.
 * Frame k is written iff k < cap_frames and off_k + ext_k <= cap_bytes; the
 * offsets are monotone, so the written frames are a prefix of W frames.
 * frames[off_k .. off_k + ext_k) holds the source's ext_k bytes; off[k] and
 * len[k] (when not NULL) are written for k < W; status = {W, bytes used
 * (off_{W-1} + ext_{W-1}, or 0), |L| - W, 0}. Nothing else is written: not the
 * gap between slot frames, not a byte past the used bytes, not off / len at
 * k >= W, no word of the batch, its lists or its records. No counter is
 * touched. A batch with n == 0 writes a zero status. */
#define COP_TX_MAX_FRAME 2048u
typedef struct cop_tx_burst {
    void     *frames;    /* device, 16-byte aligned */
    uint32_t *off;       /* device or NULL: off[k] = byte offset of frame k in frames */
    uint32_t *len;       /* device or NULL: len[k] = its length */
    uint32_t *status;    /* device, 16-byte aligned, 4 words: frames written, bytes used,
                            frames dropped (forwarded but did not fit), 0 */
    uint64_t  cap_bytes; /* < 2^32 */
    uint32_t  cap_frames;
    uint32_t  _pad;
} cop_tx_burst;
typedef struct cop_tx_desc {       /* per batch */
    const uint32_t *lens; /* IMIX batches (offsets != NULL): device, n words, frame length of
                             packet i, 1..COP_TX_MAX_FRAME; slot batches: NULL */
    uint32_t copy_bytes;  /* slot batches: bytes copied per frame, multiple of 16,
                             16 .. min(stride - data_off, COP_TX_MAX_FRAME); IMIX: 0 */
    uint32_t slot_bytes;  /* slot batches: bytes between output frames, multiple of 16,
                             >= copy_bytes; IMIX: 0 */
    cop_tx_burst out[COP_MAX_DEMUX_PORTS];
} cop_tx_desc;

/* Gather lists that exist already or are queued already (an earlier
 * cop_submit / cop_submit_ring on any lane, slots a poll-mode kernel has
 * completed). Asynchronous, on the next launch lane, ordered behind everything
 * queued before it on every lane; the outputs are valid after cop_sync. While
 * a poll-mode kernel serves the context the call is synchronous, as
 * cop_lookup_bulk is: the kernel is paused, the gather runs on the free GPU,
 * the kernel is relaunched; the outputs are valid on return.
 * nb == 0 returns 0 and launches nothing. -EINVAL (nothing launched, nothing
 * written): nb > max_batches; n > max_batch; n > 0 without pkts, fwd_idx or
 * fwd_count; a COP_CFG_NO_COMPACT context; packet starts not 16-byte aligned
 * (pkts, data_off, a stride that is no multiple of 16: 12-byte records); bad
 * copy_bytes / slot_bytes; an IMIX batch without lens, or lens / non-zero
 * copy_bytes / slot_bytes on the wrong kind; frames or status NULL or not
 * 16-byte aligned; cap_bytes >= 2^32; n * COP_TX_MAX_FRAME >= 2^32; an output
 * extent (frames, off, len, status) that overlaps any batch's packets
 * (slot batches: n * stride bytes), offsets, lens, records or lists. */
int  cop_tx_gather(cop_ctx *ctx, const cop_batch *batches, const cop_tx_desc *tx, uint32_t nb);
/* cop_submit of the batches followed by their gather, on the same lane: one
 * call, no sync in between. -EBUSY while a poll-mode kernel serves the
 * context; cop_tx_gather's and cop_submit's errors otherwise, checked before
 * anything is queued. */
int  cop_submit_tx(cop_ctx *ctx, const cop_batch *batches, const cop_tx_desc *tx, uint32_t nb);
/* The same function over host memory (every pointer a host pointer): the
 * kernel's mirror. The list layout is given explicitly: n_lists lists per
 * batch (1, or the vports of a demux layout, <= COP_MAX_DEMUX_PORTS), seg != 0
 * for segmented lists (n_lists must be 1). max_batch 0: no limit on n.
 * 0 or -EINVAL as above. */
int  cop_tx_gather_host(const cop_batch *batches, const cop_tx_desc *tx, uint32_t nb, uint32_t n_lists,
                        int seg, uint32_t max_batch);

/* ------------------------------------------------------------------------ */
/* Sketch: per-source packet accounting and policing on the device          */
/* ------------------------------------------------------------------------ */

/* A count-min sketch of the traffic: rows * cols u64 counters in device
 * memory (row r, column c at word r * cols + c, zero at creation), indexed by
 * `rows` hashes of a packet's source (or destination) address. The per-rule
 * counters (COP_CFG_RULE_COUNTERS) say nothing about a source no rule names;
 * the sketch answers "who is sending all this?" for any address, with an
 * estimate that is never below the true count.
 *
 * Key: k = addr >> (32 - key_depth), addr the packet's source
 * (COP_SKETCH_KEY_SRC) or destination (_DST) address in host byte order, read
 * where the pipeline reads it: frame bytes 26..29 / 30..33 of slot and IMIX
 * batches, record bytes 6..9 / 10..13 of COP_HDR16_STRIDE records (a batch
 * with stride 16 and no offsets). COP_HDR12_STRIDE records are -EINVAL.
 *
 * Hash: z_r = the (r+1)-th output of splitmix64 started at state = seed
 *   (state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) *
 *   0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31),
 *   a_r = (uint32_t)z_r | 1, b_r = (uint32_t)(z_r >> 32),
 *   col_r(k) = (uint32_t)(k * a_r + b_r) >> (32 - log2_cols)   (32-bit arithmetic),
 *   est(k) = min over r of counter[r][col_r(k)].
 *
 * A packet counts iff its EtherType (bytes 12..13) is 0x0800, the high nibble
 * of byte 14 is 4 (the pipeline's two checks, on the same bytes) and
 * verdict_mask == 0 or bit results[i].verdict of verdict_mask is set. */
#define COP_SKETCH_MAX_ROWS 4u
#define COP_SKETCH_KEY_SRC  0u
#define COP_SKETCH_KEY_DST  1u
typedef struct cop_sketch_config {
    uint32_t rows;       /* 1..COP_SKETCH_MAX_ROWS */
    uint32_t log2_cols;  /* 4..24: cols = 1 << log2_cols */
    uint32_t key;        /* COP_SKETCH_KEY_SRC / _DST */
    uint32_t key_depth;  /* 1..32: the key is addr >> (32 - key_depth); 32 = per host, 24 = per /24 */
    uint64_t seed;
} cop_sketch_config;
typedef struct cop_sketch cop_sketch;   /* owned by one context; several may exist */

/* Police: a batch's forward lists filtered against a threshold into new lists
 * of the same layout, which cop_tx_gather takes as they are (a cop_batch with
 * fwd_idx = out_idx, fwd_count = out_count). The lists are the context's,
 * walked as cop_tx_gather walks them (dense; one per vport with
 * COP_CFG_DEMUX_PORTS; COP_SEG_PKTS-packet segments with COP_CFG_SEG_LISTS),
 * with its clamps: a length is clamped to what the layout holds, an index
 * >= n is read as n - 1. An entry is kept iff its packet does not count as
 * IPv4 (the two header checks above; verdict_mask plays no part) or
 * est(key) < threshold. The kept entries are written, as they were read, in
 * list order: list q's at out_idx + q*n with their number at out_count[q]
 * and status[4q ..] = {kept, removed, 0, 0}; segment s's at out_idx +
 * s*COP_SEG_PKTS with their number at out_count[s], and one status for the
 * batch. Nothing of out_idx is written past a list's (segment's) kept count;
 * the batch, its lists, its records and the sketch are not written. A batch
 * with n == 0 is skipped: nothing of it is read or written. */
typedef struct cop_police_desc {
    uint64_t  threshold;  /* a list entry is kept iff its packet does not count as IPv4 or est(key) < threshold */
    uint32_t *out_idx;    /* device; the layout and capacity of the batch's fwd_idx on this context */
    uint32_t *out_count;  /* device; the layout of fwd_count */
    uint32_t *status;     /* device, 16-byte aligned; 4 words per forward list: kept, removed, 0, 0 */
} cop_police_desc;

/* -EINVAL: rows, log2_cols, key or key_depth out of range. The counters are
 * allocated and zeroed before the call returns. */
int  cop_sketch_create(cop_ctx *ctx, const cop_sketch_config *cfg, cop_sketch **out);
/* Waits for the context's queued work, then frees. cop_destroy frees the
 * sketches that are left. */
int  cop_sketch_destroy(cop_ctx *ctx, cop_sketch *sk);

/* Every call below but cop_sketch_read is asynchronous, on the next launch
 * lane, ordered behind everything queued before it on every lane (as
 * cop_tx_gather is); its outputs are valid after cop_sync. So cop_submit,
 * cop_sketch_update(1 << COP_FORWARD), cop_sketch_police, cop_tx_gather (of
 * the police's lists) need no sync between them. While a poll-mode kernel
 * serves the context every call is synchronous, as cop_lookup_bulk is: the
 * kernel is paused, the call runs and completes, the kernel is relaunched.
 * nb == 0 / n == 0 return 0 and launch nothing. -EINVAL (nothing launched,
 * nothing written): a sketch of another context; nb > max_batches; a batch
 * with n > max_batch; n > 0 without pkts (police: fwd_idx, fwd_count,
 * out_idx, out_count, status; query: ips, out); packet starts not 16-byte
 * aligned (pkts, data_off, a stride that is no multiple of 16: 12-byte
 * records), a stride of 32; verdict_mask != 0 with results NULL, or with bits
 * above COP_DROP_NO_PORT; a shift of 0 or above 64. */

/* Adds 1 to the `rows` counters of every counting packet of nb batches. Of a
 * cop_batch only pkts, offsets, n, stride, data_off and results are read
 * (results only if verdict_mask != 0). Nothing but the sketch's counters is
 * written; no pipeline counter is touched. */
int  cop_sketch_update(cop_ctx *ctx, cop_sketch *sk, const cop_batch *batches, uint32_t nb, uint32_t verdict_mask);
/* out[i] = est(ips[i] >> (32 - key_depth)): ips n u32 device words in host
 * byte order (4-byte aligned), out n u64 device words (8-byte aligned, not
 * overlapping ips or the counters). */
int  cop_sketch_query(cop_ctx *ctx, const cop_sketch *sk, const uint32_t *ips, uint32_t n, uint64_t *out);
/* One cop_police_desc per batch (above). Also -EINVAL: a COP_CFG_NO_COMPACT
 * context; status not 16-byte aligned; an output extent (out_idx, out_count,
 * status) that overlaps any batch's packets, offsets, records or lists (so
 * out_idx == fwd_idx) or the sketch's counters. */
int  cop_sketch_police(cop_ctx *ctx, const cop_sketch *sk, const cop_batch *batches, const cop_police_desc *pol,
                       uint32_t nb);
/* Ages the window: every counter >>= shift for shift 1..63; shift 64 zeroes
 * the counters. */
int  cop_sketch_decay(cop_ctx *ctx, cop_sketch *sk, uint32_t shift);
/* Synchronous: waits for the context's queued work and copies the counters to
 * host memory. Returns the word count (rows * cols), -ENOSPC if cap_words is
 * smaller, -EINVAL, -EIO. */
int  cop_sketch_read(cop_ctx *ctx, const cop_sketch *sk, uint64_t *out, uint64_t cap_words);
/* The counters in device memory, for a caller's own all-reduce (a sketch is
 * linear: the element-wise sum of two GPUs' sketches is the sketch of their
 * combined traffic) or a preload with cop_memcpy_h2d. */
int  cop_sketch_device_ptr(cop_ctx *ctx, const cop_sketch *sk, void **dptr, uint64_t *words);

/* The host mirror (csrc/sketch.c; no GPU needed): the same functions over host
 * memory, counters a caller's array of rows * cols words. The list layout is
 * explicit, as cop_tx_gather_host takes it: n_lists lists per batch, seg != 0
 * for segmented lists (n_lists must be 1), max_batch 0 for no limit on n.
 * 0 or -EINVAL as above. cop_sketch_params gives a_r and b_r of every row
 * (COP_SKETCH_MAX_ROWS words each; rows past cfg->rows are 0). */
int  cop_sketch_params(const cop_sketch_config *cfg, uint32_t a[4], uint32_t b[4]);
int  cop_sketch_update_host(const cop_sketch_config *cfg, uint64_t *counters, const cop_batch *batches, uint32_t nb,
                            uint32_t verdict_mask, uint32_t max_batch);
int  cop_sketch_query_host(const cop_sketch_config *cfg, const uint64_t *counters, const uint32_t *ips, uint32_t n,
                           uint64_t *out);
int  cop_sketch_police_host(const cop_sketch_config *cfg, const uint64_t *counters, const cop_batch *batches,
                            const cop_police_desc *pol, uint32_t nb, uint32_t n_lists, int seg, uint32_t max_batch);

/* ------------------------------------------------------------------------ */
/* AEAD: ChaCha20-Poly1305 seal / open of tx bursts on the device           */
/* ------------------------------------------------------------------------ */

/* The frames of a tx burst (what cop_tx_gather leaves: contiguous frames with
 * their off / len and a status whose word 0 is the frame count) encrypted and
 * authenticated in place with ChaCha20-Poly1305 (RFC 8439), the AEAD of
 * WireGuard and of ESP (RFC 7634). One cop_aead_burst per burst.
 *
 * Frames: k < min(*count, n_frames), or k < n_frames when count is NULL. No
 * frame at or past that number is read or written, nor its tag or ok word.
 *   l   = min(len[k], COP_TX_MAX_FRAME), or frame_bytes in the slot form
 *         (off and len both NULL);
 *   ext = (l + 15) & ~15;
 *   o   = off[k], or k * slot_bytes in the slot form (64-bit arithmetic).
 * Frame k is skipped when o is not a multiple of 16 or o + ext > cap_bytes: it
 * is counted in status word 2 and nothing of it is read or written, not its
 * tag and not its ok word. Otherwise, with a = min(aad_bytes, l):
 *   bytes [0, a) are the associated data: authenticated and left in clear (the
 *   Ethernet and IP headers the next hop must read); bytes [a, l) are the
 *   text. l == a is a valid frame: empty text, authenticated only.
 *
 * Nonce of frame k: the 12 bytes salt[0..3] || LE64(seq_base + k), the sum
 * mod 2^64. Salt zero is WireGuard's nonce, a non-zero salt RFC 7634's.
 * ChaCha20 block counter 0 gives the Poly1305 one-time key (its first 32
 * bytes); the text is XORed with the keystream from counter 1 on (at most
 * counter 32: no counter wraps). The tag is Poly1305 over
 *   AD || pad16 || ciphertext || pad16 || LE64(a) || LE64(l - a)   (RFC 8439 2.8).
 *
 * Seal encrypts [a, l) in place and writes tags[16k .. 16k+16).
 * Open computes the tag over the ciphertext, compares all 16 bytes with
 * tags[k], writes ok[k] (1 authentic and decrypted, 0 not), and decrypts in
 * place only where the tags are equal: a forged frame stays exactly as it was
 * and is counted in status word 1.
 * status = {frames processed (not skipped; open: forged ones included), open:
 * tag failures (seal: 0), frames skipped, 0}.
 *
 * What is written: after either call every byte of frames outside some
 * processed frame's [a, l) holds its previous value (the kernel may
 * read-modify-write the 16-byte pieces of a frame's own [0, ext) and touches
 * no byte outside that range); tags / ok are not written at or past the frame
 * count; off, len and count are only read. A burst with n_frames == 0 is
 * skipped whole: nothing of it is read or written, its status included.
 *
 * Reusing a (key, salt, sequence number) for two different frames is the
 * caller's misuse: it reveals the XOR of the two texts and lets tags be
 * forged. Nothing here detects it; the caller advances seq_base by the frame
 * count (n_frames is enough) from call to call. Frames that overlap inside one
 * burst (off[] not disjoint) give undefined frame contents. */
#define COP_AEAD_TAG_BYTES 16u
typedef struct cop_aead_key {
    uint8_t  key[32];
    uint8_t  salt[4];    /* nonce bytes 0..3 */
    uint32_t _pad;
} cop_aead_key;
typedef struct cop_aead_burst {
    void           *frames;     /* device, 16-byte aligned: a tx burst */
    const uint32_t *off, *len;  /* device; both or neither. Neither: frame k at k * slot_bytes, length frame_bytes */
    const uint32_t *count;      /* device or NULL: frames present = min(*count, n_frames): a tx gather's status word 0 */
    uint8_t        *tags;       /* device, 16-byte aligned, 16 bytes per frame: written by seal, read by open */
    uint32_t       *ok;         /* open: device, one word per frame (1 authentic and decrypted, 0 not); seal: NULL */
    uint32_t       *status;     /* device, 16-byte aligned, 4 words: frames processed, open: tag failures,
                                   frames skipped, 0 */
    uint64_t        cap_bytes;  /* bytes of frames[]; < 2^32 */
    uint64_t        seq_base;   /* frame k uses sequence number seq_base + k (mod 2^64) */
    uint32_t        n_frames, slot_bytes, frame_bytes, aad_bytes;
} cop_aead_burst;

/* Asynchronous, on the next launch lane, ordered behind everything queued
 * before it on every lane (as cop_tx_gather is); the outputs are valid after
 * cop_sync. So cop_submit_tx followed by cop_aead_seal of the gather's burst
 * (frames, off, len, count = the gather's status) needs no sync in between.
 * While a poll-mode kernel serves the context the call is synchronous, as
 * cop_lookup_bulk is: the kernel is paused, the call runs and completes, the
 * kernel is relaunched. The key travels as kernel arguments: there is no
 * device object and the caller's key may be reused or wiped on return.
 * nb == 0 returns 0 and launches nothing. -EINVAL (nothing launched, nothing
 * written): nb > max_batches; n_frames > max_batch; n_frames > 0 with frames,
 * tags or status NULL (open: ok); exactly one of off / len; the slot form with
 * frame_bytes 0 or above COP_TX_MAX_FRAME, or slot_bytes no multiple of 16 or
 * below frame_bytes; aad_bytes > COP_TX_MAX_FRAME; frames, tags or status not
 * 16-byte aligned (off, len, count, ok: 4-byte); cap_bytes >= 2^32; ok
 * non-NULL in seal; any overlap of an extent the call writes (frames[0,
 * cap_bytes), tags, ok, status) with any other extent of the same or another
 * burst of the call (frames, off, len, count, tags, ok, status). */
int  cop_aead_seal(cop_ctx *ctx, const cop_aead_key *key, const cop_aead_burst *bursts, uint32_t nb);
int  cop_aead_open(cop_ctx *ctx, const cop_aead_key *key, const cop_aead_burst *bursts, uint32_t nb);
/* The host mirror (csrc/aead.c; no GPU needed): the same functions over host
 * memory, every pointer a host pointer; no limit on nb or n_frames. */
int  cop_aead_seal_host(const cop_aead_key *key, const cop_aead_burst *bursts, uint32_t nb);
int  cop_aead_open_host(const cop_aead_key *key, const cop_aead_burst *bursts, uint32_t nb);
/* The building blocks, for the carry edge cases no derived key reaches.
 * cop_chacha20_block_host: one 64-byte ChaCha20 block (RFC 8439 2.3).
 * cop_poly1305_host: tag = Poly1305(otk = r || s, msg[0, n)) (RFC 8439 2.5).
 * cop_poly1305_bulk: the device's Poly1305 alone over one burst, walked as
 * above: tags[k] = Poly1305(otk[32k .. 32k+32), frame bytes [0, l)), with no
 * ChaCha and no padding or length blocks; otk is device memory, 32 bytes per
 * frame, 4-byte aligned; aad_bytes and seq_base are not used, ok is NULL;
 * status = {frames processed, 0, frames skipped, 0}. Ordering and errors are
 * cop_aead_seal's (also -EINVAL: otk NULL or overlapped by tags or status). */
void cop_chacha20_block_host(const uint8_t key[32], uint32_t counter, const uint8_t nonce[12], uint8_t out[64]);
void cop_poly1305_host(const uint8_t otk[32], const uint8_t *msg, size_t n, uint8_t tag[16]);
int  cop_poly1305_bulk(cop_ctx *ctx, const cop_aead_burst *burst, const uint8_t *otk);

/* ------------------------------------------------------------------------ */
/* L3 forward: TTL, checksum and next-hop MAC rewrite of tx bursts          */
/* ------------------------------------------------------------------------ */

/* What a router does to a frame it forwards, for batches and bursts resident
 * in device memory: the route stage's next hop (cop_result.route_nh with
 * COP_FLAG_ROUTE_HIT) indexes a neighbour table that holds the next hop's
 * MAC addresses; the TTL is decremented, the IPv4 header checksum updated
 * (RFC 1624 eqn 3) and the two MAC addresses written. cop_fwd_check filters
 * a batch's forward lists before the gather (what cannot be forwarded goes
 * to an exception list for the slow path); cop_fwd_rewrite rewrites the
 * frames of the gathered bursts in place.
 *
 * Neighbour table: one per cop_neigh, n_entries 16-byte entries in device
 * memory indexed by next hop, all zero (invalid) at creation. */
#define COP_NEIGH_VALID 0x1u
typedef struct cop_neigh_entry {
    uint8_t  dst_mac[6];  /* the next hop's address: frame bytes 0..5 */
    uint8_t  src_mac[6];  /* the egress interface's own: frame bytes 6..11 */
    uint16_t port;        /* reported in cop_fwd_rw_desc.port[] */
    uint16_t flags;       /* COP_NEIGH_VALID */
} cop_neigh_entry;
typedef struct cop_neigh cop_neigh;   /* owned by one context; several may exist */

/* n_entries 1 .. 1 << 24 (-EINVAL otherwise). The table is allocated and
 * zeroed before the call returns. */
int  cop_neigh_create(cop_ctx *ctx, uint32_t n_entries, cop_neigh **out);
/* Synchronous: waits for the context's queued work, copies host_entries[0,
 * count) to entries first .. first + count - 1 and returns. -EINVAL: a table
 * of another context, first + count > n_entries, count > 0 without
 * host_entries. Allowed while a poll-mode kernel serves the context, as
 * cop_memcpy_h2d is: that kernel never reads the table (it is paused for the
 * copy and relaunched, so the copy does not wait for its idle exit). */
int  cop_neigh_set(cop_ctx *ctx, cop_neigh *ng, uint32_t first, uint32_t count, const cop_neigh_entry *host_entries);
/* Waits for the context's queued work, then frees. cop_destroy frees the
 * tables that are left. */
int  cop_neigh_destroy(cop_ctx *ctx, cop_neigh *ng);
int  cop_neigh_device_ptr(cop_ctx *ctx, const cop_neigh *ng, void **dptr, uint32_t *n_entries);

/* Classes. A frame (b[0 ..), l bytes long) has the class of the first row
 * that applies:
 *   COP_FWD_SHORT     l < 34. Only IMIX frames can be short: l =
 *                     clamp(lens[i], 1, COP_TX_MAX_FRAME) in the check,
 *                     min(len[k], COP_TX_MAX_FRAME) in the rewrite (there
 *                     also a frame whose first 48 bytes do not lie, 16-byte
 *                     aligned, inside the burst's cap_bytes: no gather leaves
 *                     one). Nothing of a short frame is read.
 *   COP_FWD_PASS      b[12..13] != 08 00 or b[14] >> 4 != 4: not IPv4 by the
 *                     pipeline's two checks; forwarded as it is.
 *   COP_FWD_BAD_HDR   IHL (b[14] & 15) < 5
 *   COP_FWD_OPTIONS   IHL > 5: the slow path's. No byte past 33 is ever read.
 *   COP_FWD_BAD_CSUM  only with COP_FWD_VERIFY_CSUM: with w_j = b[14+2j] << 8
 *                     | b[15+2j], j = 0..9, fold(sum of w_j) != 0xFFFF; fold
 *                     adds the carries (v >> 16) back into v & 0xFFFF until
 *                     v < 0x10000.
 *   COP_FWD_TTL       b[22] <= 1
 *   COP_FWD_NO_NEIGH  nh = (results && results[i].flags & COP_FLAG_ROUTE_HIT)
 *                     ? results[i].route_nh & 0xFFFFFF : cfg.miss_nh;
 *                     nh >= n_entries or entry nh lacks COP_NEIGH_VALID.
 *                     miss_nh = COP_FWD_NO_NH puts every route miss here.
 *   COP_FWD_OK        otherwise */
#define COP_FWD_OK        0u
#define COP_FWD_PASS      1u
#define COP_FWD_SHORT     2u
#define COP_FWD_BAD_HDR   3u
#define COP_FWD_OPTIONS   4u
#define COP_FWD_BAD_CSUM  5u
#define COP_FWD_TTL       6u
#define COP_FWD_NO_NEIGH  7u
#define COP_FWD_VERIFY_CSUM 0x1u
#define COP_FWD_NO_NH     0xFFFFFFFFu
typedef struct cop_fwd_config {
    uint32_t flags;    /* COP_FWD_VERIFY_CSUM */
    uint32_t miss_nh;  /* the next hop of a packet without a route hit */
} cop_fwd_config;

/* Check: a batch's forward lists filtered into new lists of the same layout,
 * which cop_tx_gather takes as they are (cop_sketch_police's shape). The
 * lists are the context's, walked as cop_tx_gather walks them, with its
 * clamps: a length is clamped to what the layout holds, an entry e >= n is
 * read as packet i = n - 1. The class of an entry is that of packet i's
 * frame (where cop_batch puts it; of the batch's records only results[i] is
 * read, and only when results is not NULL). An entry is kept iff its class
 * is COP_FWD_OK or COP_FWD_PASS. The kept entries are written, as they were
 * read, in list order: list q's at out_idx + q*n with their number at
 * out_count[q]; segment s's at out_idx + s*COP_SEG_PKTS with their number at
 * out_count[s]. The removed entries go the same way to exc_idx / exc_count
 * (when given), each as min(e, n - 1) | class << 28. status[4q ..] = {kept,
 * removed, removed as COP_FWD_TTL, removed as COP_FWD_NO_NEIGH}; segmented
 * lists have one status per batch. Nothing of out_idx / exc_idx is written
 * past a list's (segment's) kept / removed count; the batch, its lists, its
 * records and the table are not written. A batch with n == 0 is skipped:
 * nothing of it is read or written. */
typedef struct cop_fwd_check_desc {
    const uint32_t *lens;   /* IMIX batches: device, n words (as cop_tx_desc.lens); slot batches: NULL */
    uint32_t *out_idx;      /* device; the layout and capacity of the batch's fwd_idx on this context */
    uint32_t *out_count;    /* device; the layout of fwd_count */
    uint32_t *exc_idx;      /* device or NULL (then exc_count too): the removed entries, out_idx's layout */
    uint32_t *exc_count;
    uint32_t *status;       /* device, 16-byte aligned; 4 words per forward list */
} cop_fwd_check_desc;

/* Rewrite: after cop_tx_gather of the same batches and tx. For burst q of a
 * batch (one per forward list; one per batch for segmented lists):
 *   W = min(tx.out[q].status[0], cap_frames, the list's clamped length);
 *   frame k < W is the frame of list position k (segmented lists: of the
 *   concatenation of the segments), its packet i = min(entry, n - 1), its
 *   bytes at frames + k * slot_bytes, or at frames + off[k] for IMIX.
 * The class comes from the frame's own bytes in the burst, results[i] and the
 * table. A COP_FWD_OK frame is rewritten: b[0..5] = dst_mac, b[6..11] =
 * src_mac, b[22] -= 1 and, in big-endian 16-bit words with m = b[22] << 8 |
 * b[23] (before the decrement), m' = m - 0x0100, HC = b[24] << 8 | b[25]:
 *   HC' = ~fold(~HC + ~m + m') & 0xFFFF          (RFC 1624 eqn 3)
 * into b[24..25], whether or not HC was valid. No other frame is written.
 * port[q] (when not NULL): word k < W = the entry's port for an OK frame,
 * else 0xFFFF. status[q] = {rewritten, untouched COP_FWD_PASS, untouched
 * other class, 0}. No byte of frames outside bytes [0, 26) of an OK frame
 * changes (the kernel may read-modify-write the frame's own 16-byte pieces in
 * [0, 32)); no frame at or past W is read or written, nor its port word; the
 * gather's off, len and status are only read. A batch with n == 0 is skipped.
 * Calling it twice decrements twice. */
typedef struct cop_fwd_rw_desc {
    uint32_t *port[COP_MAX_DEMUX_PORTS];     /* device or NULL: cap_frames words */
    uint32_t *status[COP_MAX_DEMUX_PORTS];   /* device, 16-byte aligned, 4 words */
} cop_fwd_rw_desc;

/* Both calls are asynchronous, on the next launch lane, ordered behind
 * everything queued before them on every lane (as cop_tx_gather and
 * cop_sketch_police are); the outputs are valid after cop_sync. So
 * cop_submit, cop_fwd_check, cop_tx_gather (of the check's lists),
 * cop_fwd_rewrite and cop_aead_seal need no sync between them. While a
 * poll-mode kernel serves the context the calls are synchronous, as
 * cop_lookup_bulk is. nb == 0 returns 0 and launches nothing.
 * -EINVAL (nothing launched, nothing written): a table of another context;
 * nb > max_batches; n > max_batch or n > 1 << 28; n > 0 with pkts, fwd_idx,
 * fwd_count, out_idx, out_count or status NULL (rewrite: a status NULL); a
 * COP_CFG_NO_COMPACT context; packet starts not 16-byte aligned (pkts,
 * data_off, stride); a slot batch's stride below 48 (16- and 32-byte
 * records); an IMIX batch without lens, or lens on a slot batch; results not
 * 8-byte aligned; status not 16-byte aligned; exactly one of exc_idx /
 * exc_count; unknown cfg.flags; in the rewrite copy_bytes < 48, an IMIX burst
 * without off and len, and every argument error of cop_tx_gather; any overlap
 * of an extent the call writes (check: out_idx, out_count, exc_idx,
 * exc_count, status; rewrite: frames[0, cap_bytes), port, status) with any
 * other extent of the call or with the table. */
int  cop_fwd_check(cop_ctx *ctx, const cop_neigh *ng, const cop_fwd_config *cfg, const cop_batch *batches,
                   const cop_fwd_check_desc *desc, uint32_t nb);
int  cop_fwd_rewrite(cop_ctx *ctx, const cop_neigh *ng, const cop_fwd_config *cfg, const cop_batch *batches,
                     const cop_tx_desc *tx, const cop_fwd_rw_desc *rw, uint32_t nb);
/* The host mirror (csrc/fwd.c; no GPU needed): the same functions over host
 * memory, entries a caller's array of n_entries entries; the list layout
 * explicit as cop_tx_gather_host takes it; max_batch 0 for no limit on n.
 * cop_ipv4_csum_host: the full recompute over a 20-byte header, bytes 10..11
 * taken as zero; returns the value whose high byte goes to byte 10. */
int  cop_fwd_check_host(const cop_neigh_entry *entries, uint32_t n_entries, const cop_fwd_config *cfg,
                        const cop_batch *batches, const cop_fwd_check_desc *desc, uint32_t nb, uint32_t n_lists,
                        int seg, uint32_t max_batch);
int  cop_fwd_rewrite_host(const cop_neigh_entry *entries, uint32_t n_entries, const cop_fwd_config *cfg,
                          const cop_batch *batches, const cop_tx_desc *tx, const cop_fwd_rw_desc *rw, uint32_t nb,
                          uint32_t n_lists, int seg, uint32_t max_batch);
uint16_t cop_ipv4_csum_host(const uint8_t hdr[20]);

/* ------------------------------------------------------------------------ */
/* ACL: 5-tuple classify and filter of batches on the device                */
/* ------------------------------------------------------------------------ */

/* A priority-ordered rule list over (source prefix, destination prefix,
 * protocol, source-port range, destination-port range): what the firewall
 * stage, one longest-prefix match on the source, cannot say ("drop TCP to
 * port 22 unless it comes from 10.1.0.0/16"). cop_acl_classify gives every
 * packet of a batch its word; cop_acl_filter, a side call of
 * cop_sketch_police's shape, removes from a batch's forward lists the entries
 * whose rule drops. The chain cop_submit -> cop_acl_filter -> cop_fwd_check
 * -> cop_tx_gather needs no sync. This is not rte_acl: the semantics are the
 * ones written here, and their ground truth is a linear scan of the rules.
 *
 * Key of a packet, from the bytes b[] where cop_batch puts it (48 readable
 * bytes; none past 37 is read). The word is exactly COP_ACL_SKIP, and nothing
 * past byte 15 is used, when b[12..13] != 08 00, b[14] >> 4 != 4 (the
 * pipeline's two checks) or (b[14] & 15) < 5. Otherwise proto = b[23],
 * src = BE32(b[26..29]), dst = BE32(b[30..33]); with (b[14] & 15) == 5 and a
 * fragment offset ((b[20] & 0x1F) << 8 | b[21]) of 0, sport = BE16(b[34..35])
 * and dport = BE16(b[36..37]) whatever the protocol; in every other case
 * (options, a later fragment) sport = dport = 0. MF alone (b[20] & 0x20, offset
 * 0) is a first fragment and has ports.
 *
 * Word of a key: a rule matches iff src and dst lie in its prefixes (depth 0:
 * any), (proto & proto_mask) == (rule.proto & proto_mask), and both ports lie
 * in its inclusive ranges. The winner is the matching rule of highest
 * priority, equal priorities the lowest index; the word is
 * index | COP_ACL_HIT | (action ? COP_ACL_DROP : 0), index the rule's position
 * in the array given to cop_acl_build. No match: exactly 0. */
#define COP_ACL_MAX_RULES 1024u
#define COP_ACL_HIT   0x01000000u   /* same bit as COP_LOOKUP_HIT */
#define COP_ACL_DROP  0x04000000u   /* same bit as COP_LOOKUP_DROP: the matching rule's action != 0 */
#define COP_ACL_SKIP  0x08000000u   /* not classified: not IPv4 by the pipeline's two checks, or IHL < 5 */
#define COP_ACL_COUNTERS 0x1u       /* cop_acl_create flag: one u64 hit counter per rule */

typedef struct cop_acl_rule {          /* 28 bytes */
    uint32_t src_ip, dst_ip;           /* host byte order, unmasked accepted (masked to the depth) */
    uint16_t sport_lo, sport_hi;       /* inclusive; lo > hi is -EINVAL */
    uint16_t dport_lo, dport_hi;
    uint8_t  src_depth, dst_depth;     /* 0..32, 0 = any address */
    uint8_t  proto, proto_mask;        /* matches iff (p & proto_mask) == (proto & proto_mask); mask 0 = any */
    int32_t  priority;                 /* the higher wins; equal priorities: the lower rule index wins */
    uint32_t action;                   /* 0 permit, non-zero drop (the firewall's convention) */
} cop_acl_rule;
typedef struct cop_acl_key { uint32_t src, dst; uint16_t sport, dport; uint8_t proto, _pad[3]; } cop_acl_key;

/* The built image, a bit-vector classifier: rules ranked by
 * (priority descending, index ascending), rank p bit p of a row of row_words
 * u32; per range field the sorted interval starts and one row per interval,
 * 256 rows for the protocol, and the rank -> word table. */
typedef struct cop_acl_report {
    uint32_t n_rules;
    uint32_t n_intervals[4];   /* src, dst, sport, dport */
    uint32_t row_words;        /* 4 * ceil(max(n, 1) / 128) */
    uint32_t first_error_idx;  /* the first bad rule (-EINVAL), n (-ENOSPC), else 0xFFFFFFFF */
    uint32_t _pad;
    uint64_t image_bytes;
} cop_acl_report;
typedef struct cop_acl_table cop_acl_table;   /* host object, no GPU needed (as cop_lpm_table) */
typedef struct cop_acl cop_acl;               /* device object, owned by one context; several may exist */

/* n may be 0 (rules may then be NULL): every key misses. rep may be NULL.
 * -EINVAL: a depth above 32, lo > hi (rep->first_error_idx the rule); -ENOSPC:
 * n > COP_ACL_MAX_RULES; -ENOMEM. Nothing is built on an error. */
int  cop_acl_build(const cop_acl_rule *rules, uint32_t n, cop_acl_table **out, cop_acl_report *rep);
void cop_acl_free(cop_acl_table *t);
/* out[i] = the word of keys[i], from the built image. */
int  cop_acl_match_host(const cop_acl_table *t, const cop_acl_key *keys, uint32_t n, uint32_t *out);

/* Uploads the image, synchronously; with COP_ACL_COUNTERS also allocates and
 * zeroes one u64 per rule. -EINVAL: unknown flags. */
int  cop_acl_create(cop_ctx *ctx, const cop_acl_table *t, uint32_t flags, cop_acl **out);
/* Waits for the context's queued work, then uploads another table's image
 * (the allocations grow if they must) and zeroes the counters. Synchronous.
 * If it fails (-ENOMEM, -EIO) the ACL holds no usable image: every call on it
 * but cop_acl_set and cop_acl_destroy is -EINVAL until a set succeeds. */
int  cop_acl_set(cop_ctx *ctx, cop_acl *acl, const cop_acl_table *t);
/* Waits for the context's queued work, then frees. cop_destroy frees the ACLs
 * that are left. */
int  cop_acl_destroy(cop_ctx *ctx, cop_acl *acl);
/* cop_rule_counters_read's contract: waits for the context's queued work,
 * copies min(cap, n_rules) words (word i: rule index i), returns n_rules (or
 * -errno); reset != 0 zeroes them after the copy. -EINVAL without
 * COP_ACL_COUNTERS. All four calls pause a poll-mode kernel, as cop_neigh_set
 * does. */
int  cop_acl_counters_read(cop_ctx *ctx, cop_acl *acl, uint64_t *out, uint32_t cap, int reset);
/* The image and the counters in device memory (counters NULL without
 * COP_ACL_COUNTERS; n_rules words, for a caller's own element-wise sum across
 * GPUs). Valid until the next cop_acl_set or cop_acl_destroy of the ACL. */
int  cop_acl_device_ptr(cop_ctx *ctx, const cop_acl *acl, void **image, uint64_t *image_bytes, void **counters,
                        uint32_t *n_rules);

/* One per batch. classify reads words; filter reads the other three. */
typedef struct cop_acl_desc {
    uint32_t *words;      /* device, n u32: classify's output */
    uint32_t *out_idx;    /* device; the layout and capacity of the batch's fwd_idx on this context */
    uint32_t *out_count;  /* device; the layout of fwd_count */
    uint32_t *status;     /* device, 16-byte aligned; 4 words per forward list: kept, removed, kept as miss, kept as skip */
} cop_acl_desc;

/* Both calls are ordered as cop_sketch_police is: asynchronous on the next
 * launch lane behind every lane's queued work, outputs valid after cop_sync;
 * synchronous beside a poll-mode kernel. nb == 0 returns 0.
 *
 * classify: words[i] = the word of packet i, for every packet of the batch.
 * Of a cop_batch only pkts, offsets, n, stride and data_off are read. Nothing
 * else is written; no counter is touched.
 *
 * filter: the context's forward lists walked with the gather's clamps (dense;
 * per vport with COP_CFG_DEMUX_PORTS; segments with COP_CFG_SEG_LISTS; an
 * entry >= n is read as n - 1, a length clamped to what the layout holds). An
 * entry is kept iff its packet's word lacks COP_ACL_DROP: misses and skipped
 * packets are kept (default deny is a depth-0 catch-all rule of lowest
 * priority). Kept entries are written as read, in list order, to out_idx /
 * out_count of the same layout, which cop_tx_gather and cop_fwd_check take as
 * they are; status[4q ..] = {kept, removed, kept as miss, kept as skip}, one
 * status per batch for segmented lists. With COP_ACL_COUNTERS every list
 * entry whose word has COP_ACL_HIT adds 1 to its rule's counter, kept or
 * removed; nothing else adds. Nothing of out_idx is written past a kept count;
 * the batch, its lists and its records are not written. A batch with n == 0
 * is skipped whole.
 *
 * -EINVAL (nothing launched, nothing written): an ACL of another context;
 * nb > max_batches; n > max_batch; n > 0 with a needed pointer NULL; packet
 * starts not 16-byte aligned; a slot batch's stride below 48; words, out_idx
 * or out_count not 4-byte aligned; in the filter a COP_CFG_NO_COMPACT context
 * and status not 16-byte aligned; any overlap of an extent the call writes
 * with any other extent of the call, the ACL's image or its counters. */
int  cop_acl_classify(cop_ctx *ctx, const cop_acl *acl, const cop_batch *batches, const cop_acl_desc *descs,
                      uint32_t nb);
int  cop_acl_filter(cop_ctx *ctx, const cop_acl *acl, const cop_batch *batches, const cop_acl_desc *descs,
                    uint32_t nb);
/* The host mirror (csrc/acl.c; no GPU needed): the same over host memory.
 * counters: n_rules u64 words or NULL (none counted). The list layout is
 * explicit, as cop_sketch_police_host takes it; max_batch 0 for no limit. */
int  cop_acl_classify_host(const cop_acl_table *t, const cop_batch *batches, const cop_acl_desc *descs, uint32_t nb,
                           uint32_t max_batch);
int  cop_acl_filter_host(const cop_acl_table *t, uint64_t *counters, const cop_batch *batches,
                         const cop_acl_desc *descs, uint32_t nb, uint32_t n_lists, int seg, uint32_t max_batch);

/* End-to-end path from host memory (NIC/KNI mbuf data): gather the first 64
 * bytes of each packet into pinned staging, hipMemcpyAsync H2D, run the
 * pipeline, hipMemcpyAsync D2H of results and forward list. Synchronous. */
int  cop_process_host(cop_ctx *ctx, const void *const *pkt_data, uint32_t n,
                      cop_result *results, uint32_t *fwd_idx, uint32_t *fwd_count);
/* Streaming form of the end-to-end path: n packets at host addresses
 * pkt_data[i], in batches of `batch` (<= max_batch): the host gather of one
 * batch overlaps the H2D copy, kernel and D2H copy of earlier batches on the
 * other lanes. results[i] for every packet. Synchronous on return. */
int  cop_process_host_stream(cop_ctx *ctx, const void *const *pkt_data, uint64_t n, uint32_t batch,
                             cop_result *results);
/* Host threads for the header gather of the two calls above: the calling
 * thread plus n-1 persistent workers (default 1 = the caller alone). */
int  cop_set_host_threads(cop_ctx *ctx, uint32_t n);

/* Asynchronous host batches (the building block of
 * cop_coprocessor_poll_async): slot s < COP_HOST_SLOTS gathers the packets'
 * 16-byte header records into its mapped pinned staging on the calling
 * thread, then queues the pipeline on launch lane s % n_streams (the kernel
 * reads the records from, and writes its results to, host memory) and
 * returns.
 * cop_host_batch_wait blocks until slot s's records are in pinned host
 * memory and points *results at them (valid until slot s is submitted
 * again). -EBUSY if the slot is still in flight. */
#define COP_HOST_SLOTS 2u
int  cop_host_batch_submit(cop_ctx *ctx, uint32_t slot, const void *const *pkt_data, uint32_t n);
int  cop_host_batch_wait(cop_ctx *ctx, uint32_t slot, const cop_result **results, uint32_t *n);

/* ------------------------------------------------------------------------ */
/* Poll-mode coprocessor: a persistent kernel serving a batch ring          */
/* ------------------------------------------------------------------------ */

/* The GPU form of the reference's coprocessor lcores, which poll their rx
 * rings forever (main_loop -> coprocessor(), switch.c:529-535) rather than
 * being started per burst. cop_pmd_start launches ONE long-lived kernel on
 * its own stream that serves `ring` (a batch ring in HBM, as for
 * cop_submit_ring) until cop_pmd_stop: the host posts batches by bumping a
 * doorbell counter in mapped host memory, and the kernel writes each batch's
 * completion back there. Batch sequence number b (0, 1, 2, ... in post
 * order) lives in ring slot b % n_slots; per-batch outputs and counters are
 * exactly those of cop_submit_ring. No launch per post: no launch latency,
 * no grid ramp, tables staged into LDS once.
 * While it runs, the context's tables cannot change (-EBUSY) and it holds
 * every worker slot it could get: another kernel is NOT guaranteed to run
 * beside it. Counters stay readable: cop_counters_read /
 * cop_counters_snapshot / cop_rule_counters_read / cop_coll_reduce_counters
 * see every completed batch (a batch's counter adds land before its
 * completion), and their reset is an atomic read-and-zero, so nothing is
 * lost or counted twice while batches run. Those that need a kernel of
 * their own (the rule-hit count, the snapshot, the RCCL all-reduce) PAUSE
 * the poll-mode kernel: it finishes every batch posted so far and leaves,
 * the side work runs, and it is relaunched (microseconds, not a wait for
 * an idle exit). Posts during a pause wait for the relaunch. One per
 * context. The kernel leaves by itself after 1 s without a post
 * ($COP_PMD_IDLE_MS) and is relaunched by the next post.
 * A ring whose pkts / results / lists live in mapped host memory must be
 * allocated coherent (cop_host_alloc_mapped does): a persistent kernel has
 * no kernel-end cache writeback, so its stores to non-coherent host pages
 * can stay in the GPU's L2. */
typedef struct cop_pmd cop_pmd;
int cop_pmd_start(cop_ctx *ctx, const cop_batch_ring *ring, cop_pmd **out);
/* Post the next `count` batches (<= n_slots): sequence numbers posted ..
 * posted+count-1. Blocks while that would reuse a slot whose batch has not
 * completed. 0 or -errno. */
int cop_pmd_post(cop_pmd *pmd, uint32_t count);
/* Spin until every batch with sequence number < seq has completed: records,
 * forward lists and counts are in HBM, visible to the host and to later
 * kernels. 0, -ETIMEDOUT (30 s) or -EIO (the kernel aborted). */
int cop_pmd_wait(cop_pmd *pmd, uint64_t seq);
uint64_t cop_pmd_posted(const cop_pmd *pmd);
/* Post `count` batches (in posts of a quarter ring, so it never drains) and
 * wait for all of them: one synchronous burst. 0 or -errno. */
int cop_pmd_run(cop_pmd *pmd, uint64_t count);
/* cop_pmd_run, stamped: CLOCK_MONOTONIC (ns) just before the first post and
 * just after the last batch is seen complete (benchmarks: the window of the
 * library call itself, no caller overhead in it). 0 or -errno. */
int cop_pmd_run_timed(cop_pmd *pmd, uint64_t count, uint64_t *t_post_ns, uint64_t *t_done_ns);
typedef struct cop_pmd_info_t {
    uint32_t workers;          /* worker workgroups (all co-resident) */
    uint32_t workers_per_cu;
    uint32_t tiles_per_batch;
    uint32_t packets_per_tile;
    uint32_t launches;         /* 1 + relaunches after idle exits */
    uint32_t state;            /* 0 running, 1 stopped, 2 left idle, 3 aborted, 4 paused */
    uint64_t posted, completed; /* summed over the rings */
    uint32_t slot_loads;       /* how tiles read their slots: 0 plain (COP_PMD_STATIC_SLOTS),
                                  3 system-coherent loads every tile (COP_PMD_SYS_ACQUIRE,
                                  host-memory rings, or slots not on 128-byte lines),
                                  4 coherent loads once the ring wraps (default); 1 and 2
                                  (acquires) only through $COP_PMD_ACQUIRE A/B runs */
    uint32_t kernel;           /* the kernel instantiation serving the rings,
                                  cop_pmd<fw, route, layout, ppt, ext>: fw table form | route form << 4
                                  | layout << 8 | ext << 12 (forms: 0 off, 1 LDS intervals, 2 DIR-24-8,
                                  3 trie, 4 bucketed; layouts: 0 slots, 1 IMIX, 2 coalesced 64 B,
                                  3 16-byte records; ppt = packets_per_tile / 256) */
} cop_pmd_info_t;
int cop_pmd_info(const cop_pmd *pmd, cop_pmd_info_t *out);
/* Complete everything posted, stop the kernel, free. */
int cop_pmd_stop(cop_pmd *pmd);

/* Several rx rings served by ONE poll-mode kernel: the GPU form of the
 * reference's five coprocessor lcores, each polling its own rx ring
 * (KNI_KTHREAD, main.c:92-94, switch.c:463). The kernel's workers are split
 * among the rings (worker w serves ring w % n_rings); each ring has its own
 * batch sequence, doorbell and completion words, so its batches complete in
 * its own order and one ring's thread never waits for another's. Every ring
 * must have ring 0's geometry (n, n_slots, stride, data_off, layout, slot
 * sizes); the pointers are each ring's own. Ring r is posted and waited by
 * one thread (different rings from different threads). At most
 * COP_PMD_MAX_RINGS. The single-ring calls above act on ring 0. */
#define COP_PMD_MAX_RINGS 8
#define COP_PMD_VARIABLE_N 1u   /* batches carry their own packet count (cop_pmd_post_batch) */
/* Slot reuse. The reference's fast path refills its rings forever
 * (switch.c:463-470), and a ring slot here may likewise be rewritten by
 * another agent (the host with cop_memcpy_h2d, a NIC, another GPU) between
 * its batches. A persistent kernel gets no dispatch-time cache invalidation,
 * so a CU or L2 could serve a slot's previous contents. By DEFAULT (no flag,
 * and always through cop_pmd_start) every tile reads its packets with
 * system-coherent loads (no cached copy used) once its ring has wrapped in
 * the running launch: a slot's first read in a launch is fresh, every reuse
 * is safe. COP_PMD_SYS_ACQUIRE: coherent loads on every tile (rings in host
 * memory get this without the flag). COP_PMD_STATIC_SLOTS: the caller
 * declares the slots written once before cop_pmd_start_rings and never again
 * while the kernel runs (a benchmark's resident pool): plain loads. The two
 * contradict (-EINVAL). */
#define COP_PMD_SYS_ACQUIRE 2u
#define COP_PMD_STATIC_SLOTS 4u
/* Dynamic tiles (rings with segmented lists, COP_CFG_SEG_LISTS): workers
 * claim tiles from ticket counters instead of a static order, and issue the
 * next tile's header loads before they classify the current one. Same
 * outputs; a higher poll-mode steady state on long streams, about the same
 * rate on short bursts. Ignored without segmented lists. */
#define COP_PMD_DYNAMIC_TILES 8u
int cop_pmd_start_rings(cop_ctx *ctx, const cop_batch_ring *rings, uint32_t n_rings, uint32_t flags,
                        cop_pmd **out);
/* Post the next `count` full batches (n packets each) of one ring. */
int cop_pmd_post_ring(cop_pmd *pmd, uint32_t ring, uint32_t count);
/* Post ONE batch of n (1..ring n) packets to one ring: the packets
 * 0..n-1 of its next slot (COP_PMD_VARIABLE_N). */
int cop_pmd_post_batch(cop_pmd *pmd, uint32_t ring, uint32_t n);
/* As cop_pmd_wait, for one ring's sequence numbers. */
int cop_pmd_wait_ring(cop_pmd *pmd, uint32_t ring, uint64_t seq);
uint64_t cop_pmd_posted_ring(const cop_pmd *pmd, uint32_t ring);
/* Batches of the ring known complete (reads the completion words). */
uint64_t cop_pmd_completed_ring(cop_pmd *pmd, uint32_t ring);

/* Counters (u64, device-resident, summed over every submitted packet).
 * On the device they are kept in COP_COUNTER_SHARDS shards of
 * COP_N_COUNTERS words (one 128-byte line each, to spread the atomics);
 * cop_counters_read folds the shards.
 * pkt_total / pkt_not_ipv4 mirror struct firewall_pkt_stats
 * (firewall.h:56-61, incremented at firewall.c:184,188); pkt_accept /
 * pkt_drop are filled here although the reference never increments them. */
typedef struct cop_counters {
    uint64_t pkt_drop;       /* DROP_FW + DROP_NOT_IPV4 (FW stage) */
    uint64_t pkt_accept;     /* FORWARD after the FW stage */
    uint64_t pkt_not_ipv4;
    uint64_t pkt_total;      /* packets that entered the FW stage */
    uint64_t parse_err;      /* DROP_PARSE (kni_interface_stats.parse_err) */
    uint64_t no_port;        /* DROP_NO_PORT */
    uint64_t forward;        /* verdict FORWARD (coprocessor tx) */
    uint64_t route_hit;      /* route LPM hits */
    uint64_t rx;             /* packets submitted */
    uint64_t _rsvd[7];
} cop_counters;
#define COP_N_COUNTERS 16
#define COP_COUNTER_SHARDS 256

int  cop_counters_read(cop_ctx *ctx, cop_counters *out, int reset);
/* Device address of the COP_COUNTER_SHARDS x COP_N_COUNTERS u64 counter
 * shards (an element-wise sum over GPUs preserves the per-shard layout). */
void *cop_counters_device_ptr(cop_ctx *ctx);

/* Per-port statistics (COP_CFG_PORT_STATS), mirroring struct
 * coprocessor_stats (switch.h:33-38) of the NF serving each vport:
 * rx_packets = packets routed to the port (enqueue_nf_rx), tx_packets =
 * packets its NF forwarded, nf_dropped = rx - tx (freed by the NF). The
 * ring-overflow drops (rx_dropped / tx_dropped) cannot occur on the device
 * path and read 0. With stage P off every packet counts as port 0. */
typedef struct cop_port_stats {
    uint64_t rx_packets;
    uint64_t rx_dropped;
    uint64_t tx_packets;
    uint64_t tx_dropped;
    uint64_t nf_dropped;
} cop_port_stats;
/* Synchronous read of min(n, n_ports) ports; returns n_ports or -errno. */
int  cop_port_stats_read(cop_ctx *ctx, cop_port_stats *out, uint32_t n, int reset);
/* Live telemetry, the read-and-zero of print_stats (switch.c:33-90), safe
 * while launches are in flight: counters (and port stats) are read — or
 * atomically exchanged with 0 when reset — by a small kernel on a separate
 * stream; no increment is lost or counted twice across snapshots. Does not
 * wait for submitted work. */
int  cop_counters_snapshot(cop_ctx *ctx, cop_counters *total, cop_port_stats *ports, uint32_t n_ports,
                           int reset);

/* Per-rule firewall hit counters (COP_CFG_RULE_COUNTERS): one u64 per rule
 * id of the firewall table (cop_lpm_export_rules order), incremented for
 * every IPv4 packet whose source matches that rule in the FW stage (the
 * rule rte_lpm_lookup resolved at firewall.c:194). Zeroed by
 * cop_set_fw_table. read: copies min(cap, n_rules) words, returns n_rules
 * (or -errno); reset != 0 zeroes them after the copy. */
int  cop_rule_counters_read(cop_ctx *ctx, uint64_t *out, uint32_t cap, int reset);
/* Device address and length of the per-rule counters. One allocation holds
 * the COP_COUNTER_SHARDS x COP_N_COUNTERS shard words, then the port-stat
 * shards (COP_COUNTER_SHARDS x 16), then the per-rule words, so one
 * element-wise u64 sum covers all three. */
int  cop_rule_counters_device_ptr(cop_ctx *ctx, void **dptr, uint32_t *n_rules);

/* Cross-GPU counter reduction over RCCL (xGMI): one communicator per
 * context, one rank per GPU. The 128-byte unique id comes from rank 0's
 * cop_coll_unique_id and is distributed by the caller (any transport).
 * librccl is loaded on first use; -ENOSYS when it is absent. */
#define COP_COLL_ID_BYTES 128
int  cop_coll_unique_id(uint8_t id[COP_COLL_ID_BYTES]);
int  cop_coll_init(cop_ctx *ctx, const uint8_t id[COP_COLL_ID_BYTES], int rank, int nranks);
/* All-reduce (u64 sum) of the counter shards and per-rule counters of every
 * rank, on the context's stream; synchronous. The sums are written to
 * *total and rule_hits[0..min(cap, n_rules)) when non-NULL (cap = 0 skips
 * the per-rule copy). reset != 0 zeroes this rank's local counters after
 * the reduction (the read-and-zero of print_stats, switch.c:33-90). */
int  cop_coll_reduce_counters(cop_ctx *ctx, cop_counters *total, uint64_t *rule_hits, uint32_t cap,
                              int reset);

/* Device memory helpers so C callers need no HIP headers. */
int  cop_dev_alloc(cop_ctx *ctx, size_t bytes, void **dptr);
/* HBM with another cache policy, for a poll-mode ring's outputs (records,
 * lists, counts) that the host or another agent reads while the kernel runs:
 * COP_ALLOC_UNCACHED (no GPU cache holds a line: a store is in memory once
 * it has drained) or COP_ALLOC_FINEGRAINED (coherent fine-grained memory).
 * Free with cop_dev_free. 0, or -errno. */
#define COP_ALLOC_UNCACHED 1u
#define COP_ALLOC_FINEGRAINED 2u
int  cop_dev_alloc_ex(cop_ctx *ctx, size_t bytes, uint32_t flags, void **dptr);
int  cop_dev_free(cop_ctx *ctx, void *dptr);
int  cop_host_alloc_pinned(cop_ctx *ctx, size_t bytes, void **hptr);
int  cop_host_free_pinned(cop_ctx *ctx, void *hptr);
/* Pinned host memory the device reads and writes coherently (mapped into
 * the device's address space; *dptr is the device's pointer to it): rings a
 * poll-mode kernel serves from host memory. Free with cop_host_free_pinned. */
int  cop_host_alloc_mapped(cop_ctx *ctx, size_t bytes, void **hptr, void **dptr);
int  cop_memcpy_h2d(cop_ctx *ctx, void *dst, const void *src, size_t bytes);
int  cop_memcpy_d2h(cop_ctx *ctx, void *dst, const void *src, size_t bytes);
int  cop_memcpy_d2d(cop_ctx *ctx, void *dst, const void *src, size_t bytes);
int  cop_memset_d(cop_ctx *ctx, void *dst, int value, size_t bytes);

/* Timing with HIP events: start/stop join every lane of the context. */
int  cop_timer_start(cop_ctx *ctx);
int  cop_timer_stop(cop_ctx *ctx, double *ms);
/* When on, every cop_submit is bracketed by an event pair; the mean kernel
 * duration of the launches since the last reset is returned in ms. */
int  cop_launch_timing(cop_ctx *ctx, int enable);
int  cop_launch_timing_read(cop_ctx *ctx, double *mean_ms, uint64_t *n, int reset);

/* ------------------------------------------------------------------------ */
/* SPSC ring with rte_ring bulk/burst semantics (init.c:74-75, switch.c)    */
/* ------------------------------------------------------------------------ */

typedef struct cop_ring cop_ring;
/* count must be a power of two; capacity is count - 1 (rte_ring default). */
cop_ring *cop_ring_create(uint32_t count);
void      cop_ring_free(cop_ring *r);
/* All-or-nothing: returns n or 0 (rte_ring_enqueue_bulk, switch.c:225,268). */
uint32_t  cop_ring_enqueue_bulk(cop_ring *r, void *const *objs, uint32_t n, uint32_t *free_space);
/* Up to n (rte_ring_dequeue_burst, switch.c:430,463). */
uint32_t  cop_ring_dequeue_burst(cop_ring *r, void **objs, uint32_t n, uint32_t *available);
uint32_t  cop_ring_count(const cop_ring *r);

/* ------------------------------------------------------------------------ */
/* Drop-in coprocessor API (coprocessor.h:23-30)                            */
/* ------------------------------------------------------------------------ */

/* rte_mbuf is opaque; the packet data address is
 * *(void **)(m + buf_addr_off) + *(uint16_t *)(m + data_off_off)
 * (rte_pktmbuf_mtod). Defaults match DPDK 17.11-19.05: 0 and 16. */
struct rte_mbuf;
void cop_set_mbuf_layout(uint32_t buf_addr_off, uint32_t data_off_off);
/* Rule file used by coprocessor_setup (coprocessor.c:19); default
 * "./nfs/firewall/rules.json", or $COP_RULE_FILE when set. */
void cop_set_rule_file(const char *path);

/* Per calling thread: create a GPU context (device = $COP_DEVICE or 0),
 * load the rule file with the reference limits. 0 or non-zero. Runs the
 * drop-in stage mask (cop_dropin_stages(), COP_STAGE_FW unless set). */
int coprocessor_setup(void);
/* The drop-in NF chain for contexts set up afterwards and for the drop-in
 * calls: COP_STAGE_FW or 0 (no NF: every packet forwards). 0 or -EINVAL. */
int cop_set_dropin_stages(uint32_t stages);
uint32_t cop_dropin_stages(void);
/* cop_set_dropin_stages(stages), then coprocessor_setup(). */
int cop_coprocessor_setup_stages(uint32_t stages);
/* coprocessor_setup() with a fixed chain: the firewall (ENABLE_FW_NF), or
 * none (DISABLE_NF). Same signature as coprocessor_setup. */
int cop_coprocessor_setup_fw(void);
int cop_coprocessor_setup_no_nf(void);
#ifndef COP_NO_DROPIN_MACROS
/* The caller's ENABLE_FW_NF / DISABLE_NF select the chain (see
 * COP_DROPIN_STAGES). An object-like alias: the reference's own declaration
 * `int coprocessor_setup(void);` (coprocessor.h:30) after this header still
 * compiles, and &coprocessor_setup is a function pointer. */
#if defined(DISABLE_NF) || defined(COP_DROPIN_NO_NF)
#define coprocessor_setup cop_coprocessor_setup_no_nf
#else
#define coprocessor_setup cop_coprocessor_setup_fw
#endif
#endif
int coprocessor_teardown(void);
/* 0 = forward, -1 = drop (coprocessor.c:50-65). One-packet GPU batch:
 * correct but latency-bound; use process_burst / cop_coprocessor_poll. */
int process_packet(struct rte_mbuf *pkt);
/* Burst form: ret[i] = process_packet(pkts[i]) for all i, one GPU batch. */
int process_burst(struct rte_mbuf **pkts, uint32_t n, int *ret);

/* Per-coprocessor counters (struct coprocessor_stats, switch.h:33-38). */
typedef struct cop_nf_stats {
    uint64_t rx_packets;
    uint64_t rx_dropped;
    uint64_t tx_packets;
    uint64_t tx_dropped;
} cop_nf_stats;

/* GPU replacement for one call of coprocessor() (switch.c:443-474): drain up
 * to max_pkts mbufs from rx in bursts of PKT_BURST_SZ, run them as one GPU
 * batch, enqueue forwarded mbufs to tx in arrival order in bulk bursts of
 * PKT_BURST_SZ (a burst that does not fit is freed and counted tx_dropped),
 * and free dropped mbufs with free_fn. Returns packets processed or -errno. */
typedef void (*cop_free_fn)(struct rte_mbuf *m, void *arg);
int cop_coprocessor_poll(cop_ctx *ctx, cop_ring *rx, cop_ring *tx, uint32_t max_pkts,
                         cop_free_fn free_fn, void *free_arg, cop_nf_stats *stats);
/* Pipelined form of cop_coprocessor_poll: each call drains up to max_pkts
 * and submits them as a GPU batch without waiting, then completes the
 * previous call's batch, forwarding and freeing exactly as
 * cop_coprocessor_poll does. So the host drains and gathers one batch while
 * the GPU runs the other. Packets leave in arrival order. Returns packets
 * completed by this call or -errno. When rx is empty, a call completes the
 * batch in flight. cop_coprocessor_flush completes everything in flight
 * (e.g. before coprocessor_teardown). */
int cop_coprocessor_poll_async(cop_ctx *ctx, cop_ring *rx, cop_ring *tx, uint32_t max_pkts,
                               cop_free_fn free_fn, void *free_arg, cop_nf_stats *stats);
int cop_coprocessor_flush(cop_ctx *ctx, cop_ring *tx, cop_free_fn free_fn, void *free_arg, cop_nf_stats *stats);
/* The calling thread's context created by coprocessor_setup (or NULL). */
cop_ctx *coprocessor_ctx(void);

/* The ring loop of several coprocessor threads on ONE poll-mode kernel (the
 * reference's five coprocessor lcores, each with its own rx ring,
 * main.c:92-94): cop_pmd_host_create starts a kernel on ctx serving n_rings
 * rings of n_slots batches of up to max_pkts packets each, whose 16-byte
 * header records and result records live in mapped pinned host memory (no
 * launch and no copy per batch), running the drop-in NF chain. Thread r then
 * calls cop_coprocessor_poll_pmd(h, r, ...) in its loop: it drains up to
 * max_pkts mbufs from rx, gathers their headers into ring r's next slot and
 * posts it; it completes (forwards to tx in arrival order, frees drops, as
 * cop_coprocessor_poll) every batch of the ring already done, oldest first,
 * and, when rx was empty or every slot is in flight, waits for the oldest.
 * Returns packets completed or -errno. cop_coprocessor_flush_pmd completes
 * everything ring r has in flight; cop_pmd_host_destroy (after every ring's
 * flush) stops the kernel. Ring r is used by one thread. */
typedef struct cop_pmd_host cop_pmd_host;
int cop_pmd_host_create(cop_ctx *ctx, uint32_t n_rings, uint32_t max_pkts, uint32_t n_slots, cop_pmd_host **out);
int cop_coprocessor_poll_pmd(cop_pmd_host *h, uint32_t ring, cop_ring *rx, cop_ring *tx, uint32_t max_pkts,
                             cop_free_fn free_fn, void *free_arg, cop_nf_stats *stats);
int cop_coprocessor_flush_pmd(cop_pmd_host *h, uint32_t ring, cop_ring *tx, cop_free_fn free_fn, void *free_arg,
                              cop_nf_stats *stats);
int cop_pmd_host_destroy(cop_pmd_host *h);

/* ------------------------------------------------------------------------ */
/* Deterministic synthetic workload (SURVEY.md §8d generator)               */
/* ------------------------------------------------------------------------ */

#define COP_GEN_FW     0  /* 1k-style firewall rule mix */
#define COP_GEN_ROUTES 1  /* BGP-like route prefix mix  */

/* Rules: splitmix64(seed). FW: 60% /24, 20% /16-23, 10% /8-15, 10% /25-32
 * confined to n_long_parents /24s; action 0 w.p. 0.5 else 1..255.
 * Routes: 55% /24, 25% /17-23, 10% /8-16, 10% /25-32; nh 1..2^24-1. */
int cop_gen_rules(uint64_t seed, uint32_t n, int kind, uint32_t n_long_parents,
                  cop_prefix *out);

typedef struct cop_trace_opts {
    uint32_t n_ports;         /* vports 192.167.10.1..n (default 5) */
    uint32_t pct_non_ipv4;    /* EtherType 0x86DD percentage (default 2) */
    uint32_t pct_bad_version; /* IPv4 EtherType, version != 4 (default 0) */
    uint32_t pct_unknown_dst; /* dst low16 in 0..4 (default 5) */
    uint32_t pct_vport_dst;   /* dst 192.167.10.x (default 60) */
    uint32_t pct_src_in_rule; /* src inside a FW rule prefix (default 50) */
} cop_trace_opts;
void cop_trace_opts_default(cop_trace_opts *o);

/* n 64-byte frames written at out + i*stride (stride >= 64). */
int cop_gen_trace(uint64_t seed, uint32_t n, const cop_trace_opts *opts,
                  const cop_prefix *fw, uint32_t n_fw,
                  const cop_prefix *routes, uint32_t n_routes,
                  uint8_t *out, uint32_t stride);
/* Simple IMIX 64/594/1518 at 7:4:1 packed into a slab at 64-byte aligned
 * offsets. Call with slab == NULL to get the slab size in *slab_bytes. */
int cop_gen_imix(uint64_t seed, uint32_t n, const cop_trace_opts *opts,
                 const cop_prefix *fw, uint32_t n_fw,
                 const cop_prefix *routes, uint32_t n_routes,
                 uint8_t *slab, uint64_t *slab_bytes, uint32_t *offsets);

#ifdef __cplusplus
}
#endif
#endif /* COP_GPU_H */
