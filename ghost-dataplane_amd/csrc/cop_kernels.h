// cop_kernels.h — launch parameters shared by the HIP runtime and the
// pipeline kernel. Internal (not part of the C ABI).
#ifndef COP_KERNELS_H
#define COP_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define COPK_BLOCK 256
#define COPK_MAXB 32
#define COPK_MAX_LAUNCH_BATCHES 1024   /* ring launches; ticket lines per lane buffer */
#define COPK_COUNTER_SHARDS 256  /* 16 u64 per shard (128 B) */
static_assert(sizeof(void *) == 8, "64-bit only");
#define COPK_LDS_MISC_WORDS 80       /* counts, tile, prefix, counter reduction */
#define COPK_LDS_MISC_EXT_WORDS 408  /* + per-port counts/prefixes (demux, port stats) */
#define COPK_COALESCED_MIN_STRIDE 48 /* coalesced loads move the first 48 bytes of every slot */
#define COPK_MAX_DEMUX_PORTS 8
#define COPK_PORT_WORDS 16           /* per shard: 8 ports x {rx, tx} */
#define COPK_STAMP_WG 65536

#define COPK_TBL_OFF 0
#define COPK_TBL_IVT 1  /* flattened intervals, binary search in LDS */
#define COPK_TBL_DIR 2  /* DIR-24-8 image in HBM */
#define COPK_TBL_TRIE 3 /* multibit trie: 12-bit top level in LDS, 6-bit popcount nodes in L2 (route stage) */
#define COPK_TBL_BKT 4  /* bucketed intervals in global memory (L2): first candidate per top-ib-bit bucket,
                           then (start, value) pairs (route stage; firewall stage with COP_CFG_FW_BKT) */
#define COPK_TRIE_L0 4096u
/* Packed tbl8 form of a DIR-24-8 image: an extended tbl24 entry's payload is
 * the offset (in 64-byte units) of its /24's run block instead of a group
 * index. A block describes the group's 256 entries as runs of equal
 * entries: 8 u64 header words h[w] = (runs starting before entry 32w) << 32
 * | bitmap of the run starts among entries 32w..32w+31, then the runs'
 * entries (u32). Entry i = value[prefix(w) + popcount(bits 0..i%32) - 1],
 * w = i/32. Blocks are 64-byte aligned: 64 + 4*runs bytes, rounded up. */

#define COPK_LAY_SLOTS 0      /* packet layouts of the one-shot kernel */
#define COPK_LAY_IMIX 1
#define COPK_LAY_COALESCED 2
#define COPK_LAY_HDR16 3      /* packed 16-byte header records (COP_HDR16_STRIDE) */

#define COPK_STAGE_PARSE 0x1u

#define COPK_FORWARD 0u
#define COPK_DROP_FW 1u
#define COPK_DROP_PARSE 2u
#define COPK_DROP_NOT_IPV4 3u
#define COPK_DROP_NO_PORT 4u
#define COPK_FLAG_ROUTE_HIT 0x1u
#define COPK_FLAG_FW_HIT 0x2u

struct CopKBatch {
    const uint8_t *pkts;
    const uint32_t *offsets;
    void *results;            // uint2 per packet
    uint32_t *fwd_idx;
    uint32_t *fwd_count;
    uint32_t n;
    uint32_t stride;
    uint32_t data_off;
    uint32_t ntiles;
};

struct CopKRing {
    const uint8_t *pkts;
    const uint32_t *offsets;
    void *results;
    uint32_t *fwd_idx;
    uint32_t *fwd_count;
    unsigned long long pkts_slot_bytes, offsets_slot_words, results_slot, fwd_slot;
    uint32_t n_slots, first, n, stride, data_off;
};

struct CopKParams {
    CopKBatch b[COPK_MAXB];                  // descriptor mode (ring == 0)
    uint32_t tile_begin[COPK_MAXB];          // first blockIdx of each batch
    uint32_t look_begin[COPK_MAXB];          // look-back word offset of each batch
    CopKRing rg;                             // ring mode (ring == 1): batch b = slot first+b
    uint32_t ring;
    uint32_t nb;
    uint32_t ntiles;
    uint32_t uniform_ntiles;  // tiles per batch when all batches are equal, else 0
    uint32_t stages;
    uint32_t n_ports;
    uint32_t compact;
    // forward lists in segments of COPK_SEG packets (COP_CFG_SEG_LISTS):
    // segment k's forward indices at fwd_idx[k*COPK_SEG ..), its length at
    // fwd_count[k]; no cross-tile prefix, so no tickets and no look-back
    uint32_t seg;
    uint32_t static_order;    // tile j of a batch = its blockIdx order (small launches: no ticket atomics)
    uint32_t epoch;
    uint32_t dbg;             // timing-only ablations ($COP_DBG), 0 in production
    // vport routing table (two-level image)
    const uint32_t *rt_top;   // 256 entries: value, or 0x80000000|leaf
    const uint16_t *rt_leaf;  // nleaf * 256
    uint32_t rt_nleaf;
    // firewall LPM. Interval form in LDS: fw_starts = fw_m sorted starts,
    // then fw_iw words of bucket index (2^fw_ib + 1 u16); fw_lv levels of
    // binary lifting inside a bucket (cop_runtime.cpp upload_lpm)
    uint32_t fw_m, fw_ib, fw_lv, fw_iw;
    const uint32_t *fw_starts, *fw_vals;
    const uint32_t *fw_tbl24, *fw_tbl8;
    uint32_t fw_tbl8_packed;  // tbl8 groups as packed run blocks (COPK_TBL8_PACKED form)
    // route LPM (the same forms)
    uint32_t lpm_m, lpm_ib, lpm_lv, lpm_iw;
    const uint32_t *lpm_starts, *lpm_vals;
    const uint32_t *lpm_tbl24, *lpm_tbl8;
    uint32_t lpm_tbl8_packed;
    uint32_t probe_nt;           // tbl24 probes as non-temporal loads (experiment, $COP_PROBE_NT)
    const uint32_t *lpm_tl0;     // trie form (lpm_trie.c): 4096 top entries (staged in LDS)
    const uint32_t *lpm_tnodes;  // 6 u32 per node: vec, leafvec (u64 each), child_base, leaf_base
    const uint32_t *lpm_tleaves;
    // bucketed form (COPK_TBL_BKT): lpm_bidx[b] = the last interval k with
    // start <= b << (32 - lpm_ib), b in [0, 2^lpm_ib] (the last entry: m - 1);
    // lpm_bpairs[2k] = start k, [2k + 1] = its value (padded with COP_BKT_PADS = 8
    // {0xFFFFFFFF, last value} pairs); lpm_lv lifting levels above the
    // widest bucket
    const uint32_t *lpm_bidx, *lpm_bpairs;
    // the firewall table in the same bucketed form (COPK_TBL_BKT firewall,
    // COP_CFG_FW_BKT: 1M-rule tables; fw_ib its index bits)
    const uint32_t *fw_bidx, *fw_bpairs;
    // LDS carve (u32 words)
    uint32_t lds_fw_off, lds_lpm_off, lds_misc_off;
    uint32_t lds_stage_off;   // one-shot kernel: the tile's forward list staged in LDS (0: none)
    uint32_t lds_rec_off;     // poll-mode kernel: the tile's records staged in LDS (0: none)
    uint32_t rec_paired;      // poll-mode kernel: records as 16-byte stores from lane pairs, no LDS stage
    // ordering / accounting state
    unsigned long long *tickets;   // one counter per batch, one 128-byte line each (zero at launch)
    unsigned long long *zero_tickets;  // the lane's other ticket buffer: zeroed by this launch
    uint32_t zero_lines;               // its dirty lines
    unsigned long long *look;
    unsigned long long *counters;
    unsigned long long *rule_hits;     // per-rule FW hit counters or nullptr
    unsigned long long *port_ctr;      // per-port {rx, tx} shards (port_stats)
    uint32_t demux;                    // > 0: one ordered forward list per port (count = ports)
    uint32_t port_stats;               // > 0: per-port counters for ports < port_stats
    uint32_t *err;
    unsigned long long *stamps;   // diagnostic phase stamps (dbg bit 8)
    // per-rule hit counters by binning (one-shot launches): each tile sorts
    // its FW hits' rule ids by bucket (id >> COPK_HIT_SHIFT) in LDS and
    // writes them to its region (runs padded to 4 ids with ~0u) plus the run
    // offsets; cop_hit_count then counts bucket by bucket in LDS and adds
    // the sums to rule_hits. hit_region == nullptr: one atomic per hit.
    uint32_t *hit_region;     // [tile][hit_reg_words]
    uint32_t *hit_off;        // [tile][hit_nb + 1]: run start of each bucket, then the end
    uint32_t hit_nb;          // buckets (<= COPK_HIT_MAX_BUCKETS)
    uint32_t hit_reg_words;   // tile * PPT*BLOCK + 4 * hit_nb
    uint32_t lds_hit_off;     // LDS: cnt[nb] | cur[nb] | wsum[4] | off[nb+1] (padded to 4) | tmp[tile] | ids[hit_reg_words]
};
#define COPK_HIT_SHIFT 14            /* 16384 rules per bucket: the count kernel's LDS counters (64 KiB) */
#define COPK_HIT_MAX_BUCKETS 256     /* 4M rules */
#define COPK_SEG 256                 /* packets per forward-list segment (= COPK_BLOCK: one tile step) */

// Poll-mode (persistent) kernel, cop_pmd.hip: n_work worker workgroups
// serve n_rings batch rings (worker w serves ring w % n_rings); every
// relay_stride-th worker of a ring relays that ring's doorbell.
#define COPK_PMD_MAX_RINGS 8
struct CopKPmd {
    CopKParams k;                        // ring mode (k.rg = ring 0, rg.first = 0), tables, counters,
                                         // options; k.uniform_ntiles = tiles per batch
    // ring r (all rings: k.rg's geometry: n, n_slots, stride, layout); each
    // ring has its own batch sequence, doorbell, gate, relays, slot counts
    // and completion words (per-ring arrays below, ring-major)
    CopKRing rings[COPK_PMD_MAX_RINGS];
    unsigned long long seq0r[COPK_PMD_MAX_RINGS];   // first batch of ring r this launch serves
    uint32_t n_rings;
    // host-mapped [r * n_slots + slot]: the packets of the batch in that
    // slot (variable-size batches, cop_pmd_post_batch), or null (every batch
    // has k.rg.n packets)
    const uint32_t *h_n;
    unsigned long long *d_act;           // device: s_memrealtime of the last doorbell change of any ring
    const unsigned long long *h_posted;  // host-mapped: batches posted (monotonic), ring r's at [8 r]
    const uint32_t *h_stop;              // host-mapped: 1 = stop, 2 = pause (leave, to be relaunched)
    // host-mapped completion: [r * n_slots + slot] = sequence + 1 of its
    // last completed batch, written by the slot's last tile (every output
    // byte of the batch, and its counter adds, landed before)
    unsigned long long *h_done;
    uint32_t *h_state;                   // host-mapped: [0] exit reason (COPK_PMD_*), [1] census
    unsigned long long *d_posted;        // device relays of ring r's posted count: COPK_PMD_RELAYS copies,
                                         // 128 B apart, ring r's at [16 (r * COPK_PMD_RELAYS + x)]
    // device: the gate, {exit reason:8 | posted:56}. Leaders publish a posted
    // count through it (CAS) before raising the relays; an exit closes it. Its
    // count then bounds the batches this launch serves: every worker finishes
    // every batch below it before leaving, none above it is started. Ring
    // r's gate at [16 r]
    unsigned long long *d_gate;
    uint32_t *d_ctl;                     // device: [0] exit (COPK_PMD_*), [1] census, [2] look-back timeout
    unsigned long long *slot_tiles;      // per (ring, slot): tiles completed (multiples of tiles per batch
                                         // between batches; zeroed at every launch), slot_stride u64 apart
    uint32_t slot_stride;                // 520 (4160 B): every counter on its own line, lines spread over
                                         // channels (packed counters cost a 20-batch burst ~3 us: tools/burst)
    unsigned long long *stamps;          // diagnostic: s_memrealtime per worker phase (COP_PMD_STAMPS) or null
    unsigned long long idle_ticks;       // s_memrealtime ticks (100 MHz) without a post before leaving
    uint32_t n_work;                     // worker workgroups
    uint32_t relay_stride;               // every relay_stride-th worker also reads the host doorbell
    uint32_t stepwise;                   // tiles step by step where tile_steps applies ($COP_PMD_STEPWISE=0: off)
    uint32_t sys_acquire;                // slot reuse: 0 plain loads (static slots); system-coherent packet
                                         // loads on every tile (3: host-memory rings) or once the ring wraps in
                                         // this launch (4: the default); A/B only: a system-scope acquire before
                                         // the loads instead, every tile (1) / once wrapped (2)
    uint32_t test_skip;                  // tests: tile test_skip - 1 of ring 0's batch 0 never runs ($COP_PMD_TEST_SKIP_TILE)
    uint32_t poll_backoff;               // waiting workers' s_sleep(4) rounds between relay polls once idle
                                         // (3: ~0.3 us, the default; 0: busy polling, $COP_PMD_BACKOFF)
    // dynamic tiles (segmented lists, step-by-step tiles): the ring's tiles
    // are claimed from a ticket counter, tile T = seq0r[r] * tiles per batch
    // + the T-th claim, instead of the static T = w + k * workers; a worker
    // claims its next tile and issues that tile's header loads before it
    // finishes the current one ($COP_PMD_DYN); 2: the same prefetch in the
    // static order, no tickets ($COP_PMD_PF)
    uint32_t dyn;
    uint32_t tk_lanes;                   // ticket lanes per ring (1, or 8: one per XCD-sized worker group)
    unsigned long long *d_ticket;        // device: ring r's lane x claim counter at [16 (r * COPK_PMD_TK_LANES + x)]
                                         // (zeroed at every launch)
};
#define COPK_PMD_TK_LANES 8
#define COPK_PMD_RELAYS 8
#define COPK_PMD_GATE_SHIFT 56
#define COPK_PMD_RUNNING 0u
#define COPK_PMD_STOPPED 1u   /* the host asked (cop_pmd_stop) */
#define COPK_PMD_IDLE 2u      /* no post for idle_ticks: left; the next post relaunches */
#define COPK_PMD_ABORT 3u     /* not every worker became resident, or a look-back timed out */
#define COPK_PMD_PAUSED 4u    /* the host asked it to make room for other kernels; relaunched after */

// cop_lpm_lookup (cop_lookup.hip): one stage's table over a stream of
// addresses. The table fields are CopKParams' for that stage, in the one
// form the launch names (COPK_TBL_IVT / DIR / TRIE / BKT).
#define COPK_LOOKUP_HIT 0x01000000u
struct CopKLookup {
    const uint32_t *ips;      // n addresses, host byte order (4-byte aligned; may equal out)
    uint32_t *out;            // n words: entry & mask on a hit, else 0
    uint32_t n;
    uint32_t ntiles;          // set by the launcher
    uint32_t mask;            // 0x01FFFFFF (next-hop image) or 0x05FFFFFF (rule-id image)
    uint32_t probe_nt;        // tbl24 probes as non-temporal loads ($COP_PROBE_NT)
    uint32_t m, ib, lv, iw;   // LDS interval image (ib: also the bucketed form's index bits)
    const uint32_t *starts, *vals;
    const uint32_t *tbl24, *tbl8;
    uint32_t tbl8_packed;
    const uint32_t *tl0, *tnodes, *tleaves;
    const uint32_t *bidx, *bpairs;
};

// The chunk grid of the side calls (cop_chunk.h): what every forward list of a
// launch says of itself, the first member of CopKTxList, CopKSkList and
// CopKFwdList. Workgroup chunk_begin + c serves the list's chunk c:
// COPK_CHUNK list positions, a segment of a segmented list.
#define COPK_CHUNK 256
struct CopKListHead {
    const uint8_t *pkts;       // batch pkts + data_off
    const uint32_t *offsets;   // IMIX: byte offset of packet i; slot batches: null
    const uint32_t *idx;       // the list's first index word (4-byte aligned)
    const uint32_t *count;     // its length (dense, per vport), or one word per segment
    uint32_t n;                // the batch's packets: what the list layout holds
    uint32_t stride;
    uint32_t chunk_begin;      // first workgroup of this list
    uint32_t _pad;
};

// cop_tx_sums / cop_tx_copy (cop_tx.hip): forwarded frames packed into tx
// bursts (cop_tx_gather). One CopKTxList per forward list (a batch's dense
// list, one vport's list, or a batch's segments in order), at most
// COPK_TX_MAXL per launch; one workgroup per chunk of COPK_TX_CHUNK list
// positions, workgroup chunk_begin + c serving the list's chunk c.
#define COPK_TX_MAXL 32
#define COPK_TX_CHUNK 256
#define COPK_TX_MAX_FRAME 2048u
struct CopKTxList {
    CopKListHead h;
    const uint32_t *lens;      // IMIX: frame length of packet i
    uint8_t *frames;           // 16-byte aligned
    uint32_t *off, *len;       // or null
    uint32_t *status;          // 16-byte aligned, 4 words
    uint32_t copy_bytes, slot_bytes;   // slot batches
    uint32_t cap_bytes, cap_frames;
    uint32_t sums_begin;       // IMIX: first word of this list's chunk byte sums in CopKTx::sums
};
struct CopKTx {
    CopKTxList l[COPK_TX_MAXL];
    uint32_t *sums;            // IMIX: context-owned scratch, one word per chunk
    uint32_t nl;
    uint32_t nchunks;          // the grid
    uint32_t seg;              // lists are segmented (COP_CFG_SEG_LISTS)
};

// cop_sketch_* (cop_sketch.hip): a count-min sketch of u64 counters in device
// memory (cop_sketch_update / query / police / decay).
#define COPK_SK_MAXB 32          /* batches per update launch */
#define COPK_SK_MAXL 32          /* forward lists per police launch */
#define COPK_SK_CHUNK 256        /* packets (update) / list positions (police) per workgroup */
#define COPK_SK_SCRATCH_WORDS 16 /* police scratch per chunk: 4 x u64 keep ballots (one per wave), kept, cnt, pad */
struct CopKSketch {
    unsigned long long *ctr;   // rows << log2_cols words
    uint32_t a[4], b[4];       // col_r(k) = (k * a[r] + b[r]) >> col_shift
    uint32_t rows;
    uint32_t log2_cols;
    uint32_t col_shift;        // 32 - log2_cols
    uint32_t key_shift;        // 32 - key_depth
    uint32_t dst;              // key on the destination address
};
struct CopKSkBatch {
    const uint8_t *pkts;       // batch pkts + data_off
    const uint32_t *offsets;   // IMIX: byte offset of packet i; else null
    const void *results;       // 8-byte records (update with a verdict mask) or null
    uint32_t n;
    uint32_t stride;           // 16: COP_HDR16_STRIDE records
    uint32_t chunk_begin;      // first workgroup of this batch
    uint32_t _pad;
};
struct CopKSkUpdate {
    CopKSketch sk;
    CopKSkBatch b[COPK_SK_MAXB];
    uint32_t nb;
    uint32_t nchunks;          // the grid
    uint32_t verdict_mask;
    uint32_t combine;          // equal keys of a workgroup combined in LDS before going to memory (0: timing A/B only)
};
struct CopKSkList {
    CopKListHead h;            // its scratch at (h.chunk_begin + c) * COPK_SK_SCRATCH_WORDS
    uint32_t *out_idx;         // the same position of the output layout
    uint32_t *out_count;
    uint32_t *status;          // 16-byte aligned, 4 words
    unsigned long long threshold;
};
struct CopKSkPolice {
    CopKSketch sk;
    CopKSkList l[COPK_SK_MAXL];
    uint32_t *scratch;         // context-owned, nchunks * COPK_SK_SCRATCH_WORDS words from scratch_begin
    uint32_t scratch_begin;    // in chunks
    uint32_t nl;
    uint32_t nchunks;          // the grid
    uint32_t seg;
};

// cop_aead_xor / cop_aead_mac / cop_aead_status (cop_aead.hip): ChaCha20-Poly1305
// over the frames of tx bursts (cop_aead_seal / _open, cop_poly1305_bulk). One
// CopKAeBurst per burst, at most COPK_AE_MAXB per launch (the parameters, the
// key included, are kernel arguments). The MAC kernel runs one frame per lane,
// COPK_AE_BLOCK frames per workgroup; the keystream kernel `group` lanes per
// frame (a power of two, 1..32), COPK_AE_BLOCK / group frames per workgroup.
#define COPK_AE_MAXB 16
#define COPK_AE_BLOCK 256
#define COPK_AE_SEAL 0u
#define COPK_AE_OPEN 1u
#define COPK_AE_POLY 2u
struct CopKAeBurst {
    uint8_t *frames;           // 16-byte aligned
    const uint32_t *off, *len; // both or neither
    const uint32_t *count;     // or null
    uint8_t *tags;             // 16-byte aligned
    uint32_t *ok;              // open
    uint32_t *status;          // 16-byte aligned, 4 words
    const uint8_t *otk;        // COPK_AE_POLY: 32 bytes per frame
    unsigned long long seq_base;
    uint32_t cap_bytes;
    uint32_t n_frames;
    uint32_t slot_bytes, frame_bytes, aad_bytes;
    uint32_t group;            // keystream kernel: lanes per frame
    uint32_t mac_begin;        // first workgroup of this burst in the MAC kernel
    uint32_t xor_begin;        // and in the keystream kernel
};
struct CopKAead {
    CopKAeBurst b[COPK_AE_MAXB];
    uint32_t key[8];           // the key's eight little-endian words
    uint32_t salt;             // nonce word 0
    uint32_t mode;             // COPK_AE_*
    uint32_t nb;
    uint32_t mac_chunks, xor_chunks;   // the two grids
    uint32_t scratch_begin;    // in MAC workgroups
    uint32_t *scratch;         // context-owned: COPK_AE_BLOCK / 64 records of 4 words per MAC workgroup, the waves'
                               // {processed, tag failures, skipped, 0}, from scratch_begin
};

// cop_fwd_mark / cop_fwd_write / cop_fwd_rw / cop_fwd_rw_status (cop_fwd.hip):
// the L3 forward step (cop_fwd_check, cop_fwd_rewrite). One CopKFwdList per
// forward list, at most COPK_FWD_MAXL per launch, on the chunk grid of
// cop_chunk.h. Scratch per chunk, COPK_FWD_SCRATCH_WORDS words from
// (scratch_begin + chunk_begin + c): check: words 0..12 the mark record,
// 16..19 the waves' COP_FWD_TTL counts, 20..23 their COP_FWD_NO_NEIGH counts,
// 24..55 the 256 4-bit classes; rewrite: words 0..2 the chunk's {rewritten,
// PASS, other}.
#define COPK_FWD_MAXL 16
#define COPK_FWD_CHUNK 256
#define COPK_FWD_SCRATCH_WORDS 56
struct CopKFwdTab {
    const uint32_t *entries;   // n_entries x 16 bytes: dst_mac, src_mac, port | flags << 16
    uint32_t n_entries;
    uint32_t verify;           // COP_FWD_VERIFY_CSUM
    uint32_t miss_nh;
    uint32_t _pad;
};
struct CopKFwdList {
    CopKListHead h;            // pkts, stride: check; offsets: rewrite takes only its being non-null
    const uint32_t *lens;      // check, IMIX: frame length of packet i
    const void *results;       // 8-byte records or null
    uint32_t *out_idx, *out_count;   // check
    uint32_t *exc_idx, *exc_count;   // check, or null
    uint32_t *status;          // 16-byte aligned, 4 words
    uint8_t *frames;           // rewrite: the burst
    const uint32_t *off, *len; // rewrite, IMIX
    const uint32_t *tx_status; // rewrite: the gather's status (word 0: frames written)
    uint32_t *port;            // rewrite, or null
    uint32_t slot_bytes;       // rewrite, slot batches
    uint32_t cap_bytes, cap_frames;   // rewrite
};
struct CopKFwd {
    CopKFwdTab tab;
    CopKFwdList l[COPK_FWD_MAXL];
    uint32_t *scratch;         // context-owned
    uint32_t scratch_begin;    // in chunks
    uint32_t nl;
    uint32_t nchunks;          // the grid
    uint32_t seg;
};

// cop_acl_words / cop_acl_mark / cop_acl_write (cop_acl.hip): the 5-tuple ACL
// (cop_acl_classify, cop_acl_filter). The image is acl.c's: per range field
// niv sorted starts and niv rows of row_words u32, 256 protocol rows and the
// rank -> word table, at word offsets that are multiples of 4. A workgroup
// stages the four starts arrays in LDS (dynamic: them, five row offsets and
// one rank per packet; the filter with counters also pad4(n_rules) words, the
// chunk's hits per rule, summed there and added to `counters` once per rule).
// Classify: one CopKAclBatch per batch, one workgroup
// per COPK_ACL_CHUNK packets. Filter: one CopKAclList per forward list on the
// chunk grid of cop_chunk.h; scratch per chunk, COPK_ACL_SCRATCH_WORDS words
// from (scratch_begin + chunk_begin + c): words 0..12 the mark record, 16..19
// the waves' kept-as-miss counts, 20..23 their kept-as-skip counts.
#define COPK_ACL_MAXB 32
#define COPK_ACL_MAXL 32
#define COPK_ACL_CHUNK 256
#define COPK_ACL_SCRATCH_WORDS 24
struct CopKAclTab {
    const uint32_t *image;         // 16-byte aligned
    unsigned long long *counters;  // filter: one per rule index, or null
    uint32_t n_rules, row_words;
    uint32_t niv[4], off_starts[4], off_rows[4];
    uint32_t off_proto, off_rank;
};
struct CopKAclBatch {
    const uint8_t *pkts;       // batch pkts + data_off
    const uint32_t *offsets;   // IMIX: byte offset of packet i; else null
    uint32_t *words;           // n words
    uint32_t n;
    uint32_t stride;
    uint32_t chunk_begin;      // first workgroup of this batch
    uint32_t _pad;
};
struct CopKAclWords {
    CopKAclTab tab;
    CopKAclBatch b[COPK_ACL_MAXB];
    uint32_t nb;
    uint32_t nchunks;          // the grid
};
struct CopKAclList {
    CopKListHead h;
    uint32_t *out_idx;         // the same position of the output layout
    uint32_t *out_count;
    uint32_t *status;          // 16-byte aligned, 4 words
};
struct CopKAcl {
    CopKAclTab tab;
    CopKAclList l[COPK_ACL_MAXL];
    uint32_t *scratch;         // context-owned
    uint32_t scratch_begin;    // in chunks
    uint32_t nl;
    uint32_t nchunks;          // the grid
    uint32_t seg;
};

#ifdef __cplusplus
extern "C" {
#endif
hipError_t copk_acl_words_launch(const CopKAclWords *p, hipStream_t stream);
hipError_t copk_acl_filter_launch(const CopKAcl *p, hipStream_t stream);
hipError_t copk_fwd_check_launch(const CopKFwd *p, hipStream_t stream);
hipError_t copk_fwd_rewrite_launch(const CopKFwd *p, hipStream_t stream);
// seal: keystream, MAC, status; open: MAC (writes ok), keystream under ok, status; poly: MAC, status
hipError_t copk_aead_launch(const CopKAead *p, hipStream_t stream);
hipError_t copk_sketch_update_launch(const CopKSkUpdate *p, hipStream_t stream);
hipError_t copk_sketch_police_launch(const CopKSkPolice *p, hipStream_t stream);
hipError_t copk_sketch_query_launch(const CopKSketch *sk, const uint32_t *ips, uint32_t n, unsigned long long *out,
                                    hipStream_t stream);
// every counter >>= shift (1..63), or 0 (64)
hipError_t copk_sketch_decay_launch(const CopKSketch *sk, uint32_t shift, hipStream_t stream);
// imix: every list is of an IMIX batch (the byte-sum pre-pass runs first), or none is
hipError_t copk_tx_launch(const CopKTx *p, int imix, hipStream_t stream);
// form: COPK_TBL_*; the grid is min(tiles, ncu x resident workgroups per CU,
// grid_cap if non-zero)
hipError_t copk_lookup_launch(const CopKLookup *p, int form, uint32_t ncu, uint32_t grid_cap, hipStream_t stream);
hipError_t copk_pmd_launch(const CopKPmd *p, int fw_mode, int lpm_mode, int layout, int ppt, int ext,
                           uint32_t lds_bytes, hipStream_t stream);
// resident workgroups per CU of that kernel at lds_bytes (the occupancy API)
hipError_t copk_pmd_occupancy(int fw_mode, int lpm_mode, int layout, int ppt, int ext, uint32_t lds_bytes,
                              int *per_cu);
// layout: COPK_LAY_*
hipError_t copk_launch(const CopKParams *p, int fw_mode, int lpm_mode, int layout, int ppt,
                       uint32_t grid, uint32_t lds_bytes, hipStream_t stream);
// per-rule hit counters from the binned ids of n_tiles tiles (see hit_region)
hipError_t copk_hit_count(const CopKParams *p, uint32_t n_tiles, uint32_t tile_pkts, hipStream_t stream);
// dst[i] = src[i] (atomic load) or atomic exchange with 0 when reset
hipError_t copk_snapshot(unsigned long long *src, uint32_t n_words, unsigned long long *dst, int reset,
                         hipStream_t stream);
// cop_lpm_patch (cop_patch.hip): n disjoint fill records {table, first, count,
// entry} (device memory, 16 bytes each, count <= COPK_PATCH_SPAN) written into
// tbl24 (cap24 entries) and tbl8 (cap8 entries); both bases 16-byte aligned.
// A record that leaves its table is skipped, never written in part.
#define COPK_PATCH_SPAN 1024u
hipError_t copk_patch_launch(const void *recs, uint32_t n, uint32_t *tbl24, uint32_t cap24, uint32_t *tbl8,
                             uint32_t cap8, hipStream_t stream);
// cop_lpm_paint (cop_paint.hip): a whole DIR-24-8 image from niv sorted
// intervals (starts[0] == 0, entries: the device entry of each) and the
// ascending list of the n_ext extended /24 blocks, all device memory: every
// one of the 2^24 tbl24 entries, tbl8 groups 0 .. n_ext - 1, zeros in groups
// n_ext .. cap_groups - 1, nothing beyond cap_groups * 256. One workgroup per
// COPK_PAINT_CHUNK consecutive blocks, then one wave per tbl8 group. tbl24 and
// tbl8 16-byte aligned; n_ext <= cap_groups.
#define COPK_PAINT_CHUNK 4096u
hipError_t copk_paint_launch(const uint32_t *starts, const uint32_t *entries, uint32_t niv, const uint32_t *ext24,
                             uint32_t n_ext, uint32_t *tbl24, uint32_t *tbl8, uint32_t cap_groups, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
