"""Batches whose every packet has a prescribed verdict class and port.

The generator's traffic forwards about half of each batch at random, so the
code that turns verdicts into outputs (csrc/cop_device.h: compact_tile in
its three forms, look_back / look_back_seg / lb_publish, copy_out_list,
st_list_chunk, seg_epilogue, store_records_paired, copy_out_records, the
four counter reductions; csrc/cop_tile.h: emit / flush of tile_steps_v)
never meets a tile, segment, wave or chunk whose forward count is 0, 1,
full or a given residue mod 4. This module builds the inputs that
test_verdict_patterns.py (the builder against the oracle, on the host) and
test_gpu_verdict_patterns.py (the kernels against the prescription) share:

  fw_rules / route_rules / routing_table   tiny tables that stay in LDS
  frames        64-byte frames whose packet i has exactly the prescribed
                class, port and route outcome, with the records and the
                nine counters that follow from the prescription alone
  patterns      named boolean forward masks of a batch of n packets in
                tiles of T = 256 * PPT packets
  classes_of    a mask turned into classes (the drop class rotates with i)
  dense_list, seg_lists, port_lists, port_stats, rule_hits
                the expected lists and statistics, in plain numpy
"""
import numpy as np

import copgpu as cg
import lpm_edges as le

S, F, L = cg.STAGE_PARSE, cg.STAGE_FW, cg.STAGE_LPM
SEG = cg.SEG_PKTS

# verdict classes
FWD_HIT, FWD_MISS, DROP_FW, PARSE_ETH, PARSE_DST, NOT_IPV4, NO_PORT = range(7)
CLASS_NAMES = ["FWD_HIT", "FWD_MISS", "DROP_FW", "PARSE_ETH", "PARSE_DST", "NOT_IPV4", "NO_PORT"]
DROP_CLASSES = (DROP_FW, PARSE_ETH, PARSE_DST, NOT_IPV4, NO_PORT)
VERDICT_OF = np.array([cg.FORWARD, cg.FORWARD, cg.DROP_FW, cg.DROP_PARSE, cg.DROP_PARSE, cg.DROP_NOT_IPV4,
                       cg.DROP_NO_PORT], dtype=np.uint8)
REACHED = np.array([1, 1, 1, 0, 0, 1, 0], dtype=bool)       # classes that enter the firewall stage

# firewall: rule ids 0..5 in this order; 10.(1+r).0.0/16 and two /24s inside misses' neighbours
FW_IP = [0x0A010000, 0x0A020000, 0x0A030300, 0x0A040000, 0x0A050500, 0x0A060000]
FW_DEPTH = [16, 16, 24, 16, 24, 16]
FW_ACTION = [1, 0, 7, 0, 255, 0]
FW_DROP_RULES = [0, 2, 4]
FW_ACCEPT_RULES = [1, 3, 5]
FW_CFG = (1024, 24, True)
SRC_MISS = 0x0B000000                                        # 11.0.0.0/8: no rule

# route stage (S | F | L): 20.0.0.0/8 and 20.1.0.0/16 inside it; 30.0.0.0/8 misses
ROUTE_IP = [0x14000000, 0x14010000]
ROUTE_DEPTH = [8, 16]
ROUTE_NH = [0x000111, 0x0ABCDE]
DST_HIT = (0x14020000, 0x14010000)                           # -> ROUTE_NH[0], ROUTE_NH[1]
DST_MISS = 0x1E000000

# vport routing table keys (dst & 0xFFFF): port q at PORT_KEY[q], in eight different leaves
PORT_KEY = [0x4000 + 0x111 * q for q in range(cg.MAX_DEMUX_PORTS)]
NO_PORT_KEY, NO_PORT_VALUE = 0x5005, 200                     # a port >= any n_ports
UNKNOWN_KEY = 0x6006                                         # UNKNOWN_PORT


def fw_rules() -> np.ndarray:
    return le.rows(FW_IP, FW_DEPTH, FW_ACTION)


def route_rules() -> np.ndarray:
    return le.rows(ROUTE_IP, ROUTE_DEPTH, ROUTE_NH)


def routing_table(n_ports: int = 5) -> np.ndarray:
    rt = cg.route_table_default(n_ports)
    for q in range(cg.MAX_DEMUX_PORTS):
        rt[PORT_KEY[q]] = q
    rt[NO_PORT_KEY] = NO_PORT_VALUE
    rt[UNKNOWN_KEY] = cg.UNKNOWN_PORT
    return rt


def frames(classes, ports, route_hit=None, stages=S | F):
    """(frames, records, counters) of len(classes) packets: packet i has
    class classes[i]; the classes that pass the parse stage are routed to
    vport ports[i]; with route_hit (a boolean mask, stage L on) the packets
    that pass the parse stage hit (alternately one of two route prefixes) or
    miss the route table. Records and counters come from the prescription."""
    cl = np.asarray(classes, dtype=np.int64)
    n = len(cl)
    i = np.arange(n, dtype=np.uint64)
    ports = np.asarray(ports, dtype=np.int64)
    assert len(ports) == n and (ports >= 0).all() and (ports < cg.MAX_DEMUX_PORTS).all()
    assert (stages & (S | F)) == (S | F)
    lpm = bool(stages & L)
    assert lpm == (route_hit is not None)
    # source: picks the firewall outcome; low bits vary inside the rule
    rule = np.full(n, -1, dtype=np.int64)
    d, a = np.array(FW_DROP_RULES), np.array(FW_ACCEPT_RULES)
    rule[cl == DROP_FW] = d[(i[cl == DROP_FW] // np.uint64(7)) % np.uint64(len(d))]
    rule[cl == FWD_HIT] = a[(i[cl == FWD_HIT] // np.uint64(7)) % np.uint64(len(a))]
    base = np.where(rule >= 0, np.array(FW_IP, dtype=np.uint64)[np.maximum(rule, 0)], np.uint64(SRC_MISS))
    span = np.where(rule >= 0, np.uint64(1) << (np.uint64(32) - np.array(FW_DEPTH, dtype=np.uint64)[np.maximum(rule, 0)]),
                    np.uint64(1 << 24))
    src = base + (i * np.uint64(2654435761)) % span
    # destination: low 16 bits pick the vport, the rest the route outcome
    key = np.array(PORT_KEY, dtype=np.uint64)[ports]
    key[cl == PARSE_DST] = UNKNOWN_KEY
    key[cl == NO_PORT] = NO_PORT_KEY
    which = (i // np.uint64(3)) % np.uint64(2)
    if lpm:
        rh = np.asarray(route_hit, dtype=bool)
        top = np.where(rh, np.array(DST_HIT, dtype=np.uint64)[which], np.uint64(DST_MISS))
    else:
        rh = np.zeros(n, dtype=bool)
        top = np.full(n, 0xC0A70000, dtype=np.uint64)
    dst = top | key
    pk = le.probe_frames(src.astype(np.uint32), dst.astype(np.uint32))
    f = pk.reshape(n, 64)
    f[cl == PARSE_ETH, 12] = 0x86
    f[cl == PARSE_ETH, 13] = 0xDD
    f[cl == NOT_IPV4, 14] = 0x65
    # records
    reached = REACHED[cl]
    rec = np.zeros(n, dtype=cg.RESULT_DT)
    rec["verdict"] = VERDICT_OF[cl]
    rec["port"] = np.where(reached, ports, np.where(cl == NO_PORT, NO_PORT_VALUE, cg.UNKNOWN_PORT))
    fw_hit = (cl == FWD_HIT) | (cl == DROP_FW)
    rec["flags"] = fw_hit * cg.FLAG_FW_HIT + (rh & reached) * cg.FLAG_ROUTE_HIT
    rec["route_nh"] = np.where(rh & reached, np.array(ROUTE_NH, dtype=np.uint32)[which], 0)
    return pk, rec, counters(cl, rh if lpm else None)


def counters(classes, route_hit=None) -> dict:
    """The nine counters (cop_counters) of a batch, from its classes."""
    cl = np.asarray(classes)
    cnt = np.bincount(cl, minlength=7)
    fwd = int(cnt[FWD_HIT] + cnt[FWD_MISS])
    return {"pkt_drop": int(cnt[DROP_FW] + cnt[NOT_IPV4]), "pkt_accept": fwd, "pkt_not_ipv4": int(cnt[NOT_IPV4]),
            "pkt_total": int(REACHED[cl].sum()), "parse_err": int(cnt[PARSE_ETH] + cnt[PARSE_DST]),
            "no_port": int(cnt[NO_PORT]), "forward": fwd,
            "route_hit": 0 if route_hit is None else int((np.asarray(route_hit, bool) & REACHED[cl]).sum()),
            "rx": len(cl)}


def add_counters(*cs) -> dict:
    return {k: sum(c[k] for c in cs) for k in cg.COUNTER_NAMES}


def rule_hits(classes) -> np.ndarray:
    """Per-rule firewall hits (rule id order) of frames(classes, ...)."""
    cl = np.asarray(classes)
    i = np.arange(len(cl))
    out = np.zeros(len(FW_IP), dtype=np.uint64)
    for c, ids in ((DROP_FW, FW_DROP_RULES), (FWD_HIT, FW_ACCEPT_RULES)):
        r = np.array(ids)[(i[cl == c] // 7) % len(ids)]
        out += np.bincount(r, minlength=len(FW_IP)).astype(np.uint64)
    return out


# ---------------------------------------------------------------------------
# forward masks

def edge_positions(n: int, T: int) -> list:
    return sorted({p for p in (0, 1, 63, 64, 255, 256, T - 1, T, n - 1) if 0 <= p < n})


def patterns(n: int, T: int) -> dict:
    """name -> boolean forward mask of n packets in tiles of T."""
    i = np.arange(n)
    one = np.ones(n, dtype=bool)
    seg, tile = i // SEG, i // T
    nt = int(tile[-1]) + 1
    out = {"none": ~one, "all": one.copy()}
    for p in edge_positions(n, T):
        out[f"one_fwd@{p}"] = i == p
        out[f"one_drop@{p}"] = i != p
    out["even"] = i % 2 == 0
    out["odd"] = i % 2 == 1
    for name, unit in (("wave", i // 64), ("seg", seg), ("tile", tile)):
        out[f"alt_{name}"] = unit % 2 == 0
        out[f"alt_{name}_inv"] = unit % 2 == 1
    k = 1 + seg % 7
    seg_len = np.minimum(SEG, n - seg * SEG)
    out["seg_head_k"] = i % SEG < k
    out["seg_tail_k"] = i % SEG >= seg_len - k
    out["first_tile_only"] = tile == 0
    out["last_tile_only"] = tile == nt - 1
    out["one_per_tile"] = i % T == tile % T
    out["tile_head_k"] = i % T < 2 + tile % 7           # tile aggregates 2, 3, 4, ...: every residue mod 4
    out["bern_1_64"] = np.random.default_rng(0x5EED7A01).random(n) < 1 / 64
    out["bern_63_64"] = np.random.default_rng(0x5EED7A02).random(n) < 63 / 64
    for c in DROP_CLASSES:
        out[f"none:{CLASS_NAMES[c]}"] = ~one
    for m in out.values():
        m.setflags(write=False)
    return out


LONG_CHAIN = ("first_tile_only", "last_tile_only", "alt_tile", "alt_tile_inv", "all", "none")
WHOLE = ("all", "none", "odd", "seg_tail_k", "last_tile_only", "one_per_tile", "bern_63_64")
DEMUX_MASKS = ("all", "even", "alt_tile", "bern_1_64")
ROUTE_CASES = ("all", "none", "even", "alt_wave", "seg_head_k", "bern_1_64", "one_drop@63", "none:NOT_IPV4")
LONG_N = 257 * 256 + 1         # 258 tiles of 256: a second look-back round


def ragged(T: int) -> int:
    """Three whole tiles and a tail that is odd, no multiple of 4 and ends 3 packets into a segment."""
    return 3 * T + 259


def shapes() -> list:
    """(n, T, pattern names or None for all) of every batch shape the GPU tests run."""
    out = []
    for T in (256, 1024, 2048):
        out += [(ragged(T), T, None), (3 * T, T, WHOLE)]
    return out + [(LONG_N, 256, LONG_CHAIN)]


def route_hit_mask(n: int) -> np.ndarray:
    """A fixed-seed mask independent of every forward mask: about 5 in 8 hit."""
    return np.random.default_rng(0x5EED7A03).random(n) < 0.625


def select(n: int, T: int, names=None) -> dict:
    p = patterns(n, T)
    return p if names is None else {k: p[k] for k in names}


def classes_of(name: str, fwd: np.ndarray) -> np.ndarray:
    """Classes of a forward mask: forwards alternate between a firewall hit
    with action 0 and a miss, drops rotate with i over the five drop classes
    (pattern "none:CLASS": that class alone)."""
    n = len(fwd)
    i = np.arange(n)
    cl = np.where((i // 3) % 2 == 0, FWD_HIT, FWD_MISS)
    drop = np.array(DROP_CLASSES)[i % len(DROP_CLASSES)]
    if ":" in name:
        drop = np.full(n, CLASS_NAMES.index(name.split(":")[1]))
    return np.where(fwd, cl, drop)


# ---------------------------------------------------------------------------
# expectations

def nseg(n: int) -> int:
    return (n + SEG - 1) // SEG


def dense_list(fwd) -> np.ndarray:
    return np.nonzero(fwd)[0].astype(np.uint32)


def seg_lists(fwd):
    """(counts per segment, list per segment) of a forward mask."""
    fwd = np.asarray(fwd, dtype=bool)
    lists = [np.nonzero(fwd[s * SEG:(s + 1) * SEG])[0].astype(np.uint32) + np.uint32(s * SEG)
             for s in range(nseg(len(fwd)))]
    return np.array([len(x) for x in lists], dtype=np.uint32), lists


def port_lists(fwd, ports, K: int):
    """(counts per port, list per port) for K vports."""
    fwd, ports = np.asarray(fwd, dtype=bool), np.asarray(ports)
    lists = [np.nonzero(fwd & (ports == q))[0].astype(np.uint32) for q in range(K)]
    return np.array([len(x) for x in lists], dtype=np.uint32), lists


def port_stats(classes, ports, K: int) -> np.ndarray:
    """K x (rx, tx): packets routed to each vport and packets it forwarded."""
    cl, ports = np.asarray(classes), np.asarray(ports)
    reached, fwd = REACHED[cl], VERDICT_OF[cl] == cg.FORWARD
    return np.array([[int((reached & (ports == q)).sum()), int((fwd & (ports == q)).sum())] for q in range(K)],
                    dtype=np.int64)


def port_layouts(n: int, T: int, K: int) -> dict:
    """name -> port of every packet, all below K."""
    i = np.arange(n)
    out = {"port0": np.zeros(n, dtype=np.int64), "mod": i % K, "wave": (i // 64) % K, "tile": (i // T) % K}
    if K > 1:
        out[f"port{K - 1}"] = np.full(n, K - 1, dtype=np.int64)
    return out
