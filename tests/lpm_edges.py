"""Tables and probe sets that put every device LPM lookup on its edges.

The host tests sweep every prefix boundary through numpy or C mirrors of the
lookups; the kernels (csrc/cop_device.h: ivt_value / ivt_search, tbl8_step,
tbl8_issue / tbl8_finish, trie_walk, bkt_step, bkt_pairs_issue /
bkt_pairs_finish) are separately written code. This module builds the inputs
that test_lpm_edges.py (their intended structure, on the host) and
test_gpu_lpm_edges.py (the kernels against the oracle) share:

  boundary_probes   first and last address of every accepted rule, the
                    address either side of each, and the ends of the space
  probe_frames      valid 64-byte IPv4 frames carrying given (src, dst)
  bkt_widths        buckets of the bucketed form holding exactly 1..19, 31,
                    32 and 33 boundaries (the w > 7 cut, odd and even ends of
                    the wide-bucket rounds)
  stride_edges      all-zero and all-ones paths at every depth 8..32 (child
                    63 of every trie node, child 3 of the 2-bit last level),
                    tbl8 runs that change at entries 31 / 32 / 33, a group of
                    256 distinct entries
  lds_limit         host routes up to and past the LDS interval limit
  small_tables      tables that stay in LDS, among them the empty table and
                    the two ends of the address space

Rule sets are PREFIX_DT arrays; fw_rules() turns one into a firewall rule
set whose neighbouring rules alternate between FORWARD and DROP_FW.
"""
import numpy as np

import copgpu as cg

FORM_NH, FORM_RULE = 0, 1
IVT_MAX = 8192                      # cop_runtime.cpp: LDS interval entries per table
BKT_TARGETS = list(range(1, 20)) + [31, 32, 33]
RT_CFG = (1 << 20, 1 << 16, False)  # max_rules, number_tbl8s, stop_at_first_error


def rows(ip, depth, next_hop) -> np.ndarray:
    return cg.prefixes(np.asarray(ip, dtype=np.uint64), depth, next_hop)


def boundary_probes(table, extra=None) -> np.ndarray:
    """Sorted unique u32 addresses lo-1, lo, lo+1, hi-1, hi, hi+1 of every
    accepted rule of `table` (an LpmTable, or its rules()), wrapping mod
    2^32, plus 0, 1, 0xFFFFFFFE and 0xFFFFFFFF (and `extra`). Rule edges,
    not intervals(): the firewall's rule-id image keeps breakpoints that the
    next-hop image merges away."""
    r = table.rules() if hasattr(table, "rules") else table
    depth = r["depth"].astype(np.uint64)
    span = (np.uint64(1) << (np.uint64(32) - depth)) - np.uint64(1)   # depth 0: the whole space
    lo = r["ip"].astype(np.uint64) & ~span & np.uint64(0xFFFFFFFF)
    hi = lo | span
    one = np.uint64(1)
    parts = [lo + np.uint64(0xFFFFFFFF), lo, lo + one, hi + np.uint64(0xFFFFFFFF), hi, hi + one,
             np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint64)]
    if extra is not None:
        parts.append(np.asarray(extra, dtype=np.uint64))
    return np.unique(np.concatenate(parts) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def subsample(probes: np.ndarray, cap: int = 200000, seed: int = 0x5EED0E01) -> np.ndarray:
    """At most `cap` of the probes (fixed seed), the four ends of the space kept."""
    if len(probes) <= cap:
        return probes
    keep = np.random.default_rng(seed).choice(len(probes), cap - 4, replace=False)
    return np.unique(np.concatenate([probes[keep], probes[:2], probes[-2:]]))


def pad_to(probes: np.ndarray, multiple: int) -> np.ndarray:
    """The probes, repeated from the start up to a multiple of `multiple`."""
    n = -(-len(probes) // multiple) * multiple
    return probes[np.arange(n) % len(probes)]


def probe_frames(src, dst=None, seed: int = 0x5EED0E00) -> np.ndarray:
    """len(src) valid 64-byte IPv4 frames (EtherType 0x0800, version 4) as
    the trace generator writes them, with bytes 26..29 = src and 30..33 =
    dst, big-endian. dst defaults to src reversed, so one batch sweeps the
    firewall (source) and the route stage (destination) with every probe."""
    src = np.ascontiguousarray(src, dtype=np.uint32)
    dst = src[::-1] if dst is None else np.ascontiguousarray(dst, dtype=np.uint32)
    assert len(src) == len(dst)
    n = len(src)
    pk = cg.gen_trace(seed, n, None, None,
                      opts=cg.trace_opts(pct_non_ipv4=0, pct_bad_version=0, pct_unknown_dst=0))
    f = pk.reshape(n, 64)
    f[:, 26:30] = src.astype(">u4").view(np.uint8).reshape(-1, 4)
    f[:, 30:34] = dst.astype(">u4").view(np.uint8).reshape(-1, 4)
    return pk


def write_headers(slab: np.ndarray, offs: np.ndarray, src, dst):
    """The same (src, dst) written into an IMIX slab's frames at their offsets."""
    o = offs.astype(np.int64)[:, None] + np.arange(4)
    slab[o + 26] = np.ascontiguousarray(src, dtype=np.uint32).astype(">u4").view(np.uint8).reshape(-1, 4)
    slab[o + 30] = np.ascontiguousarray(dst, dtype=np.uint32).astype(">u4").view(np.uint8).reshape(-1, 4)


def filler() -> np.ndarray:
    """30k random routes without 10/8..13/8 (left to the crafted rules): keeps
    a table above IVT_MAX intervals, so the trie and bucketed forms are used."""
    r = cg.gen_rules(0x5EED2098, 30000, cg.GEN_ROUTES, 0)
    top = r["ip"] >> 24
    return r[(top < 10) | (top > 13)]


def bkt_cluster_offsets(w: int) -> list:
    """Offsets of /32 host routes from a bucket's first address that put
    exactly w boundaries inside the bucket: a host at offset 0 adds one (its
    end; its start is the bucket's), a host at 4, 7, 10, ... adds two."""
    offs = [0] if w & 1 else []
    return offs + [4 + 3 * j for j in range(w // 2)]


def bkt_widths_crafted() -> np.ndarray:
    ip, nh = [], []
    for i, w in enumerate(BKT_TARGETS):
        base = 0x0A000000 | ((96 + i) << 16)        # 10.(96+i).0.0: a bucket start for any ib <= 24
        for o in bkt_cluster_offsets(w):
            ip.append(base + o)
            nh.append(0x010000 + (i << 8) + o)
    return rows(ip, 32, nh)


def bkt_widths() -> np.ndarray:
    return np.concatenate([filler(), bkt_widths_crafted()])


STRIDE_EXTRA = np.arange(0x0D000000, 0x0D000400, dtype=np.uint32)   # 13.0.0.0 .. 13.0.3.255, every address


def stride_edges_crafted() -> np.ndarray:
    ip, depth, nh = [], [], []
    for d in range(8, 33):
        mask = (0xFFFFFFFF << (32 - d)) & 0xFFFFFFFF
        ip += [0x0B000000, 0x0CFFFFFF & mask]       # all-zero path, all-ones path
        depth += [d, d]
        nh += [0x020000 + d, 0x030000 + d]
    for o in (0, 1, 31, 32, 33, 63, 64, 255):       # runs of a packed tbl8 group changing around a word
        ip.append(0x0D000000 + o)
        depth.append(32)
        nh.append(0x040000 + o)
    for o in range(256):                             # a group of 256 distinct entries
        ip.append(0x0D000100 + o)
        depth.append(32)
        nh.append(0x050000 + o)
    ip.append(0x0D000280)                            # 13.0.2.128/25
    depth.append(25)
    nh.append(0x060000)
    return rows(ip, depth, nh)


def stride_edges() -> np.ndarray:
    return np.concatenate([filler(), stride_edges_crafted()])


def lds_limit(h: int) -> np.ndarray:
    """h /32 routes, no two adjacent, 0.0.0.0 among them: 2h intervals."""
    k = np.arange(h, dtype=np.uint64)
    return rows((np.uint64(2 * 1000003) * k) & np.uint64(0xFFFFFFFF), 32, 1 + k)


def small_tables() -> dict:
    """name -> (rules, LpmTable configuration): tables for the LDS form."""
    return {
        "crafted": (stride_edges_crafted(), RT_CFG),
        "empty": (rows([], [], []), RT_CFG),
        "halves": (rows([0, 0x80000000], [1, 1], [7, 9]), RT_CFG),
        "ends": (rows([0, 0xFFFFFFFF], [32, 32], [5, 6]), RT_CFG),
        "fw1k": (cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20), (1024, 24, True)),
    }


def routes100k() -> np.ndarray:
    return cg.gen_rules(0x5EED2003, 100000, cg.GEN_ROUTES, 0)


def fw_rules(rules: np.ndarray) -> np.ndarray:
    """The same prefixes as firewall rules: action index % 2, so DROP_FW and
    FORWARD alternate across neighbouring rules."""
    out = rules.copy()
    out["next_hop"] = np.arange(len(rules)) % 2
    return out


def table(rules: np.ndarray, cfg=RT_CFG) -> cg.LpmTable:
    max_rules, tbl8s, stop = cfg
    return cg.LpmTable(rules, max(max_rules, len(rules), 1), tbl8s, stop)


def interval_search(tab: cg.LpmTable, ips: np.ndarray):
    """(next hop, hit) of each address by binary search over intervals()."""
    s, v = tab.intervals()
    e = v[np.searchsorted(s, np.asarray(ips, dtype=np.uint32), "right") - 1]
    return e & 0x00FFFFFF, ((e >> 24) & 1).astype(np.uint8)


def lds_index(starts: np.ndarray):
    """numpy restatement of the LDS interval image's index (cop_runtime.cpp
    upload_lpm): (M, ib, idx, lv) for a table of m = len(starts) intervals."""
    m = len(starts)
    M = 4
    while M < m:
        M *= 2
    srt = np.full(M, 0xFFFFFFFF, dtype=np.uint64)
    srt[:m] = starts
    ib = 0
    while (1 << ib) < m and ib < 12:
        ib += 1
    ib = max(ib, 6)
    nb = 1 << ib
    x = np.arange(nb + 1, dtype=np.uint64) << np.uint64(32 - ib)
    x[nb] = 0xFFFFFFFF
    # R(x): the last k with srt[k] <= x; the end sentinel R(0xFFFFFFFF) is M - 1 (the pads)
    idx = np.searchsorted(srt, x, "right") - 1
    widest = int(np.diff(idx).max())
    lv = 0
    while (1 << lv) <= widest:
        lv += 1
    return M, ib, idx, lv


def bucket_widths(tab: cg.LpmTable, bucket_starts, form: int = FORM_NH) -> np.ndarray:
    """Boundaries inside the bucketed form's bucket (idx[b + 1] - idx[b]) at
    each of bucket_starts, from intervals() and the form's bucket bits."""
    s, _ = tab.intervals()
    ib = tab.bkt_probe(np.zeros(1, np.uint32), form)[2]["ib"]
    b0 = np.asarray(bucket_starts, dtype=np.uint64)
    assert not (b0 & np.uint64((1 << (32 - ib)) - 1)).any()
    edges = np.stack([b0, b0 + np.uint64(1 << (32 - ib))], axis=1)
    k = np.searchsorted(s.astype(np.uint64), edges, "right") - 1
    return np.diff(k, axis=1)[:, 0]
