"""Vport routing tables and batches that probe every key of them.

cop_set_routing_table compresses the 65536-entry table into rt_top[256] plus
one 256-entry leaf per non-uniform block; stage_tables brings rt_top and
rt_nleaf * 32 16-byte chunks into LDS in 1 KiB pieces, and pass1 reads
rt_leaf[(top & 0xFFFF) << 8 | idx & 0xFF]. The tables here put that image on
its edges (0, 1, 3, 128, 255 and 256 leaves; a leaf in block 0 and in block
255; a block whose only differing entry is its first, second, last but one
or last; uniform blocks whose value has bit 15 set), and the batch looks up
every one of the 65536 keys once, in a fixed permutation, followed by 512
frames that the parse stage must judge before the table. This module is
shared by test_route_cases.py (the oracle against the derivation below, on
the host) and test_gpu_route_lds.py (the kernels against the same).

  TABLES / table(name)   the routing tables, with their leaf counts
  leaf_count(rt)         the leaf count of any table, in numpy
  frames()               the batch (one for all tables): 64-byte slots
  expected(rt, stages)   records, forward mask and counters, in plain numpy
  imix / hdr16 / hdr12   the same frames in the other three layouts
"""
import functools
from collections import namedtuple

import numpy as np

import copgpu as cg
import lpm_edges as le
import verdict_patterns as vp

S, F, L = vp.S, vp.F, vp.L
N_PORTS = 5
N_KEYS = 65536
N_TAIL = 512
N = N_KEYS + N_TAIL

# the values a block or a leaf entry takes: the five ports, two ports beyond
# them, a value with bit 15 alone, the largest port number, UNKNOWN_PORT
VALUES = np.array([0, 1, 2, 3, 4, 5, 200, 0x8000, 0xFFFE, 0xFFFF], dtype=np.uint16)
# name -> leaves (non-uniform blocks) of the table's two-level image
TABLES = {"uniform": 0, "first": 1, "last": 1, "three": 3, "odd_blocks": 128, "all_but_one": 255, "all": 256}
UNIFORM_MIDDLE = 127          # all_but_one: the one uniform block

# the tail: keys of four blocks (0 and 255 are leaves in first / last, 1 in
# odd_blocks, 128 in three; all four in all_but_one and all), each with a
# frame the parse stage drops or hands on whatever the table holds
TAIL_BLOCKS = (0, 255, 1, 128)


def _uniform() -> np.ndarray:
    return np.repeat(VALUES[np.arange(256) % len(VALUES)], 256)


def _random_block(rng) -> np.ndarray:
    blk = VALUES[rng.integers(0, len(VALUES), 256)]
    assert len(np.unique(blk)) > 1
    return blk


@functools.lru_cache(maxsize=None)
def table(name: str) -> np.ndarray:
    """The named table (read-only)."""
    rt = _uniform()
    rng = np.random.default_rng(0x5EED7B00 + list(TABLES).index(name))
    if name == "first":
        rt[0] = 3                             # block 0 (value 0) differs in entry 0 alone
    elif name == "last":
        rt[0xFFFF] = 2                        # block 255 (value 5) differs in entry 255 alone
    elif name == "three":
        rt[1] = 4                             # block 0: entry 1 alone
        rt[128 * 256:129 * 256] = _random_block(rng)
        rt[0xFFFE] = 1                        # block 255: entry 254 alone
    elif name in ("odd_blocks", "all_but_one", "all"):
        for b in range(256):
            if (name == "odd_blocks" and b % 2 == 0) or (name == "all_but_one" and b == UNIFORM_MIDDLE):
                continue
            rt[b * 256:(b + 1) * 256] = _random_block(rng)
    else:
        assert name == "uniform"
    rt.setflags(write=False)
    return rt


def leaf_count(rt) -> int:
    b = np.asarray(rt).reshape(256, 256)
    return int((b != b[:, :1]).any(axis=1).sum())


# ---------------------------------------------------------------------------
# frames

Frames = namedtuple("Frames", "pk key eth_ok ver_ok rule route")


@functools.lru_cache(maxsize=None)
def frames() -> Frames:
    """N 64-byte frames: packet i < 65536 is IPv4, version 4, with
    dst & 0xFFFF = perm[i]; the last 512 carry keys of TAIL_BLOCKS with
    EtherType 0x86DD (even) or version nibble 6 (odd). Sources cycle over the
    six rules of verdict_patterns' firewall and a miss, the upper half of the
    destination over its two route prefixes and a miss.
    key, eth_ok, ver_ok: per packet; rule: the firewall rule id or -1;
    route: index into vp.ROUTE_NH or -1."""
    i = np.arange(N, dtype=np.uint64)
    perm = np.random.default_rng(0x5EED7BFF).permutation(N_KEYS).astype(np.uint64)
    j = np.arange(N_TAIL, dtype=np.uint64)
    per = N_TAIL // len(TAIL_BLOCKS)
    tail = np.array(TAIL_BLOCKS, dtype=np.uint64)[j // np.uint64(per)] * np.uint64(256) + \
        (j * np.uint64(151)) % np.uint64(256)
    key = np.concatenate([perm, tail])
    rule = ((i // np.uint64(5)) % np.uint64(7)).astype(np.int64)
    rule[rule == 6] = -1
    r0 = np.maximum(rule, 0)
    base = np.where(rule >= 0, np.array(vp.FW_IP, dtype=np.uint64)[r0], np.uint64(vp.SRC_MISS))
    span = np.where(rule >= 0, np.uint64(1) << (np.uint64(32) - np.array(vp.FW_DEPTH, dtype=np.uint64)[r0]),
                    np.uint64(1 << 24))
    src = base + (i * np.uint64(2654435761)) % span
    route = (i % np.uint64(3)).astype(np.int64)
    route[route == 2] = -1
    top = np.where(route >= 0, np.array(vp.DST_HIT, dtype=np.uint64)[np.maximum(route, 0)], np.uint64(vp.DST_MISS))
    dst = top | key
    pk = le.probe_frames(src.astype(np.uint32), dst.astype(np.uint32))
    f = pk.reshape(N, 64)
    eth_ok, ver_ok = np.ones(N, dtype=bool), np.ones(N, dtype=bool)
    eth_ok[N_KEYS::2] = False
    ver_ok[N_KEYS + 1::2] = False
    f[~eth_ok, 12] = 0x86
    f[~eth_ok, 13] = 0xDD
    f[~ver_ok, 14] = 0x65
    out = Frames(pk, key.astype(np.int64), eth_ok, ver_ok, rule, route)
    for a in out:
        a.setflags(write=False)
    return out


Expected = namedtuple("Expected", "rec fwd cnt")


def expected(rt, stages: int, n_ports: int = N_PORTS) -> Expected:
    """What the header rules give for frames() under table rt
    (get_next_hop, switch.c:93-136; the port bound, switch.c:316-319;
    fw_packet_handler, firewall.c:170-213): port = rt[dst & 0xFFFF], or
    UNKNOWN_PORT for a non-IPv4 EtherType; 0xFFFF -> DROP_PARSE,
    >= n_ports -> DROP_NO_PORT; the packets left enter the firewall (a
    version nibble other than 4 -> DROP_NOT_IPV4, else the rule's action)
    and the route stage."""
    assert stages & S
    fr = frames()
    rt = np.asarray(rt, dtype=np.uint16)
    port = np.where(fr.eth_ok, rt[fr.key], cg.UNKNOWN_PORT).astype(np.int64)
    verdict = np.full(N, cg.FORWARD, dtype=np.int64)
    verdict[port == cg.UNKNOWN_PORT] = cg.DROP_PARSE
    verdict[(port != cg.UNKNOWN_PORT) & (port >= n_ports)] = cg.DROP_NO_PORT
    reached = verdict == cg.FORWARD
    flags = np.zeros(N, dtype=np.int64)
    nh = np.zeros(N, dtype=np.int64)
    cnt = dict.fromkeys(cg.COUNTER_NAMES, 0)
    if stages & F:
        not4 = reached & ~fr.ver_ok
        looked = reached & fr.ver_ok
        action = np.array(vp.FW_ACTION)[np.maximum(fr.rule, 0)]
        drop = looked & (fr.rule >= 0) & (action != 0)
        verdict[not4] = cg.DROP_NOT_IPV4
        verdict[drop] = cg.DROP_FW
        flags[looked & (fr.rule >= 0)] |= cg.FLAG_FW_HIT
        cnt["pkt_total"] = int(reached.sum())
        cnt["pkt_not_ipv4"] = int(not4.sum())
        cnt["pkt_drop"] = int(not4.sum() + drop.sum())
        cnt["pkt_accept"] = int((looked & ~drop).sum())
    if stages & L:
        hit = reached & (fr.route >= 0)
        flags[hit] |= cg.FLAG_ROUTE_HIT
        nh[hit] = np.array(vp.ROUTE_NH)[fr.route[hit]]
        cnt["route_hit"] = int(hit.sum())
    fwd = verdict == cg.FORWARD
    cnt["parse_err"] = int((port == cg.UNKNOWN_PORT).sum())
    cnt["no_port"] = int(((port != cg.UNKNOWN_PORT) & (port >= n_ports)).sum())
    cnt["forward"] = int(fwd.sum())
    cnt["rx"] = N
    rec = np.zeros(N, dtype=cg.RESULT_DT)
    rec["verdict"], rec["flags"], rec["port"], rec["route_nh"] = verdict, flags, port, nh
    rec.setflags(write=False)
    fwd.setflags(write=False)
    return Expected(rec, fwd, cnt)


def rule_hits(rt, n_ports: int = N_PORTS) -> np.ndarray:
    """Per-rule firewall hits (rule id order) of frames() under rt."""
    fr = frames()
    e = expected(rt, S | F, n_ports)
    hit = (e.rec["flags"] & cg.FLAG_FW_HIT) != 0
    return np.bincount(fr.rule[hit], minlength=len(vp.FW_IP)).astype(np.uint64)


def port_lists(e: Expected, K: int = N_PORTS):
    """(counts per port, list per port): the forwards of each vport, ascending."""
    return vp.port_lists(e.fwd, np.minimum(e.rec["port"], K), K)


def port_stats(e: Expected, K: int = N_PORTS) -> np.ndarray:
    """K x (rx, tx): packets routed to each vport and packets it forwarded."""
    p = e.rec["port"]
    return np.array([[int((p == q).sum()), int((e.fwd & (p == q)).sum())] for q in range(K)], dtype=np.int64)


# ---------------------------------------------------------------------------
# layouts

IMIX_GAPS = (64, 80, 128, 208, 64, 320, 96, 112)       # bytes from one frame's start to the next: multiples of 16


@functools.lru_cache(maxsize=None)
def imix():
    """(slab, offsets): the frames at 16-byte aligned offsets of an IMIX slab
    (each frame's first 64 bytes; the gaps between them hold 0xEE)."""
    fr = frames()
    gaps = np.array(IMIX_GAPS, dtype=np.int64)[np.arange(N) % len(IMIX_GAPS)]
    offs = np.concatenate([[0], np.cumsum(gaps)[:-1]])
    slab = np.full(int(offs[-1]) + 64 + 64, 0xEE, dtype=np.uint8)
    slab[offs[:, None] + np.arange(64)] = fr.pk.reshape(N, 64)
    offs = offs.astype(np.uint32)
    slab.setflags(write=False)
    offs.setflags(write=False)
    return slab, offs


@functools.lru_cache(maxsize=None)
def hdr16() -> np.ndarray:
    """16-byte header records: frame bytes 12..15 and 24..35."""
    out = cg.pack_headers_np(frames().pk, N)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hdr12() -> np.ndarray:
    """12-byte header records: frame bytes 12..15 and 26..33."""
    f = frames().pk.reshape(N, 64)
    out = np.ascontiguousarray(np.concatenate([f[:, 12:16], f[:, 26:34]], axis=1)).reshape(-1)
    out.setflags(write=False)
    return out


LAYOUTS = ("slots", "imix", "hdr16", "hdr12")


def layout(name: str):
    """(bytes, stride, offsets or None) of the frames in the named layout."""
    if name == "slots":
        return frames().pk, 64, None
    if name == "imix":
        slab, offs = imix()
        return slab, 0, offs
    if name == "hdr16":
        return hdr16(), cg.HDR16_STRIDE, None
    assert name == "hdr12"
    return hdr12(), cg.HDR12_STRIDE, None
