"""Inputs and expectations the ACL tests share (test_acl_host.py on the host,
test_gpu_acl.py on the device).

The restatement of include/cop_gpu.h ("ACL") in numpy: `keys_of` takes a
packet's key from its bytes, `scan` gives a key's word by a linear scan of the
rules in (priority descending, index ascending) order. Neither looks at the
built image. `edge(n)` and `mixed()` are the rule sets with their probe keys.

An AclCase holds one batch in plain numpy: frames whose every byte is random
except the fields set on purpose, forward lists in one of the three list forms
(tx_cases.lay_lists), and the outputs (words, out_idx, out_count, status)
between 0xAB guards. Every case carries the fixed pattern of header kinds
KIND_PATTERN. It has sketch_cases.SkCase's shape, so sketch_cases.host_descs
and sketch_cases.Pack (one device buffer whose whole image is compared) take it.
"""
import numpy as np

import copgpu as cg
import tx_cases as tc

GUARD, PAD, SEG = tc.GUARD, tc.PAD, cg.SEG_PKTS
HIT, DROP, SKIP = cg.ACL_HIT, cg.ACL_DROP, cg.ACL_SKIP
EDGE_NS = (0, 1, 31, 32, 33, 127, 128, 129, 1023, 1024)
EDGE_RANKS = (0, 31, 32, 127, 128)
# name -> (stride, data_off); stride 0: IMIX offsets
LAYOUTS = {"s64": (64, 0), "s128": (128, 0), "s2176": (2176, 128), "imix": (0, 16)}
KINDS = ("plain", "et86dd", "ver6", "ihl4", "ihl6", "frag1", "mf0")
# the kind of packet i is KIND_PATTERN[i % 16]: most packets are plain, every other kind comes once in 16
KIND_PATTERN = ("plain", "et86dd", "plain", "ver6", "plain", "ihl4", "plain", "ihl6", "plain", "frag1", "plain", "mf0",
                "plain", "plain", "plain", "plain")


# ---- the restatement ---------------------------------------------------------------------------------------
def keys_of(pk: np.ndarray, starts: np.ndarray):
    """(skipped, keys) of the packets that start at `starts`; a skipped packet's key is all zero."""
    s = starts.astype(np.int64)
    b = lambda o: pk[s + o].astype(np.uint32)
    be32 = lambda o: (b(o) << 24) | (b(o + 1) << 16) | (b(o + 2) << 8) | b(o + 3)
    be16 = lambda o: (b(o) << 8) | b(o + 1)
    skip = (b(12) != 0x08) | (b(13) != 0x00) | ((b(14) >> 4) != 4) | ((b(14) & 15) < 5)
    has_ports = ((b(14) & 15) == 5) & ((((b(20) & 0x1F) << 8) | b(21)) == 0)
    k = np.zeros(len(s), dtype=cg.ACL_KEY_DT)
    k["proto"] = np.where(skip, 0, b(23))
    k["src"], k["dst"] = np.where(skip, 0, be32(26)), np.where(skip, 0, be32(30))
    k["sport"] = np.where(skip | ~has_ports, 0, be16(34))
    k["dport"] = np.where(skip | ~has_ports, 0, be16(36))
    return skip, k


def seen_kinds(pk: np.ndarray, starts: np.ndarray) -> set:
    """The header kinds among the packets, from their bytes."""
    s = starts.astype(np.int64)
    b = lambda o: pk[s + o].astype(np.uint32)
    et_ok, v4, ihl = (b(12) == 0x08) & (b(13) == 0x00), (b(14) >> 4) == 4, b(14) & 15
    off, mf = ((b(20) & 0x1F) << 8) | b(21), (b(20) & 0x20) != 0
    out = set()
    for name, m in (("et86dd", ~et_ok), ("ver6", et_ok & ~v4), ("ihl4", et_ok & v4 & (ihl < 5)),
                    ("ihl6", et_ok & v4 & (ihl > 5)), ("frag1", et_ok & v4 & (ihl == 5) & (off != 0)),
                    ("mf0", et_ok & v4 & (ihl == 5) & (off == 0) & mf),
                    ("plain", et_ok & v4 & (ihl == 5) & (off == 0) & ~mf)):
        if m.any():
            out.add(name)
    return out


def order_of(rules: np.ndarray) -> list:
    """Rule indices in (priority descending, index ascending) order: position p is rank p."""
    return sorted(range(len(rules)), key=lambda i: (-int(rules["priority"][i]), i))


def matches(r, keys: np.ndarray) -> np.ndarray:
    """Which keys rule r matches."""
    def prefix(ip, depth, addr):
        mask = np.uint32((0xFFFFFFFF << (32 - int(depth))) & 0xFFFFFFFF) if depth else np.uint32(0)
        return (addr & mask) == (np.uint32(ip) & mask)
    pm = np.uint8(r["proto_mask"])
    return (prefix(r["src_ip"], r["src_depth"], keys["src"]) & prefix(r["dst_ip"], r["dst_depth"], keys["dst"]) &
            ((keys["proto"] & pm) == (np.uint8(r["proto"]) & pm)) &
            (keys["sport"] >= r["sport_lo"]) & (keys["sport"] <= r["sport_hi"]) &
            (keys["dport"] >= r["dport_lo"]) & (keys["dport"] <= r["dport_hi"]))


def scan(rules: np.ndarray, keys: np.ndarray) -> np.ndarray:
    """The word of every key: the first rule in order_of that matches, or 0."""
    words = np.zeros(len(keys), dtype=np.uint32)
    open_ = np.ones(len(keys), dtype=bool)
    for i in order_of(rules):
        m = open_ & matches(rules[i], keys)
        words[m] = i | HIT | (DROP if rules["action"][i] else 0)
        open_ &= ~m
    return words


def make_keys(src, dst, sport, dport, proto) -> np.ndarray:
    n = len(np.atleast_1d(src))
    k = np.zeros(n, dtype=cg.ACL_KEY_DT)
    k["src"], k["dst"], k["sport"], k["dport"], k["proto"] = src, dst, sport, dport, proto
    return k


# ---- the rule sets -----------------------------------------------------------------------------------------
EDGE_SRC = 0x0A000000


def edge(n: int):
    """(rules, probe keys): rule i a distinct source /32 with a scrambled priority (rank != index, with ties)
    and one lowest-priority catch-all in the middle of the array. The probes hit ranks 0, 31, 32, 127, 128 and
    n - 1 (the catch-all) where they exist; every probe also matches the catch-all."""
    rules = cg.acl_rules(n)
    rng = np.random.default_rng(0xACE0 + n)
    if n:
        i = np.arange(n)
        rules["src_ip"], rules["src_depth"] = EDGE_SRC + 3 * i, 32
        rules["priority"] = (i * 37) % 11 - 3
        rules["action"] = (i % 3 == 0).astype(np.uint32) * (1 + i)
        ca = n // 2
        rules["src_ip"][ca], rules["src_depth"][ca], rules["priority"][ca], rules["action"][ca] = 0, 0, -1000, 7
    order = order_of(rules)
    if n > 2:
        assert order != list(range(n)) and len(set(rules["priority"].tolist())) < n
    ranks = [r for r in EDGE_RANKS if r < n - 1] + ([n - 1] if n else [])
    src = [int(rules["src_ip"][order[r]]) if r < n - 1 else 0xC0000201 for r in ranks]
    src += [EDGE_SRC + 1, 0, 0xFFFFFFFF] + [EDGE_SRC + 3 * int(x) for x in rng.integers(0, max(n, 1), 8)]
    m = len(src)
    keys = make_keys(src, rng.integers(0, 1 << 32, m, dtype=np.uint64), rng.integers(0, 1 << 16, m),
                     rng.integers(0, 1 << 16, m), rng.integers(0, 256, m))
    if n:
        assert order[n - 1] == n // 2                                        # the catch-all is the last rank
        w = scan(rules, keys[:len(ranks)])
        assert [int(x) & 0xFFFFFF for x in w] == [order[r] for r in ranks]   # the probes hit those ranks
    return rules, keys


MIXED_N = 200


def mixed():
    """(rules, keys): about 200 rules over every field form, and for every rule each field at lo, hi, lo - 1
    and hi + 1 where they exist (the other fields inside the rule), the fields' extremes, and random keys."""
    rng = np.random.default_rng(0xAC1)
    n = MIXED_N
    rules = cg.acl_rules(n)
    depths = np.array([0, 1, 8, 16, 24, 31, 32])
    pool = np.array([0x0A010203, 0x0A01FF00, 0xC0A80001, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF, 0x00000000, 0x0A020000],
                    dtype=np.uint64)
    for f in ("src", "dst"):
        rules[f + "_ip"] = pool[rng.integers(0, len(pool), n)] ^ rng.integers(0, 256, n).astype(np.uint64)
        rules[f + "_depth"] = depths[rng.integers(0, len(depths), n)]
    fixed = [(0, 0), (65535, 65535), (0, 65535), (22, 22), (80, 80), (1024, 65535), (0, 1023), (65534, 65535), (0, 1)]
    for f in ("sport", "dport"):
        for i in range(n):
            if rng.random() < 0.7:
                lo, hi = fixed[rng.integers(0, len(fixed))]
            else:
                lo = int(rng.integers(0, 65536))
                hi = lo if rng.random() < 0.5 else int(rng.integers(lo, 65536))
            rules[f + "_lo"][i], rules[f + "_hi"][i] = lo, hi
    rules["proto"] = np.array([6, 17, 1, 0x2F, 0x60, 0xFF])[rng.integers(0, 6, n)]
    rules["proto_mask"] = np.array([0, 0xFF, 0xF0])[rng.integers(0, 3, n)]
    rules["priority"] = np.array([-5, 0, 1, 7, 1000])[rng.integers(0, 5, n)]
    rules["action"] = rng.integers(0, 2, n)

    rows = []
    for r in rules:
        rng_of = {}
        for f in ("src", "dst"):
            d = int(r[f + "_depth"])
            mask = (0xFFFFFFFF << (32 - d)) & 0xFFFFFFFF if d else 0
            lo = int(r[f + "_ip"]) & mask
            rng_of[f] = (lo, lo | (~mask & 0xFFFFFFFF), 0xFFFFFFFF)
        for f in ("sport", "dport"):
            rng_of[f] = (int(r[f + "_lo"]), int(r[f + "_hi"]), 0xFFFF)
        base = {f: v[0] for f, v in rng_of.items()}
        base["proto"] = int(r["proto"])
        rows.append(dict(base))
        for f, (lo, hi, top) in rng_of.items():
            for v in (lo, hi, lo - 1, hi + 1, 0, top):
                if 0 <= v <= top:
                    rows.append(dict(base, **{f: v}))
        for v in (int(r["proto"]) ^ 0x01, int(r["proto"]) ^ 0x10, 0, 255):
            rows.append(dict(base, proto=v))
    keys = make_keys(*(np.array([x[f] for x in rows], dtype=np.uint64) for f in ("src", "dst", "sport", "dport", "proto")))
    m = 512
    rand = make_keys(rng.integers(0, 1 << 32, m, dtype=np.uint64), rng.integers(0, 1 << 32, m, dtype=np.uint64),
                     rng.integers(0, 1 << 16, m), rng.integers(0, 1 << 16, m), rng.integers(0, 256, m))
    return rules, np.concatenate([keys, rand])


def traffic_rules(n: int, seed: int = 0) -> np.ndarray:
    """n generated rules for traffic of addresses 10.x: prefixes of 10/8 of mixed depths, a few port and
    protocol conditions, and a lowest-priority permit-all, so that frames hit, miss nothing and some drop."""
    rng = np.random.default_rng(0xAC7 + seed)
    r = cg.acl_rules(n)
    if not n:
        return r
    r["src_ip"] = 0x0A000000 | rng.integers(0, 1 << 24, n)
    r["src_depth"] = np.array([8, 12, 16, 20, 24, 32])[rng.integers(0, 6, n)]
    r["dst_depth"] = np.array([0, 0, 8, 16])[rng.integers(0, 4, n)]
    r["dst_ip"] = 0x0A000000 | rng.integers(0, 1 << 24, n)
    low = rng.random(n) < 0.3
    r["dport_hi"] = np.where(low, 1023, 0xFFFF)
    r["proto"], r["proto_mask"] = 6, np.where(rng.random(n) < 0.25, 0xFF, 0)
    r["priority"] = rng.integers(0, 8, n)
    r["action"] = rng.integers(0, 2, n)
    r[n - 1] = cg.acl_rules(1)[0]
    r["priority"][n - 1] = -1
    return r


# ---- one batch ---------------------------------------------------------------------------------------------
class AclCase:
    """One batch, its forward lists and the outputs of both calls. keys: the 5-tuples the frames carry,
    cycled (default: random ones); the header kind of packet i is KIND_PATTERN[i % 16]."""

    def __init__(self, n, layout="s64", form="dense", fwd=None, K=1, seed=0, keys=None):
        self.n, self.layout, self.form, self.K = n, layout, form, K
        self.n_lists, self.seg = (K if form == "demux" else 1), form == "seg"
        self.stride, self.data_off = LAYOUTS[layout]
        self.imix = self.stride == 0
        rng = np.random.default_rng(0xAC15E + 131 * seed + n)
        m = max(n, 1)
        if self.imix:
            offsets = (rng.permutation(m) * 64).astype(np.uint32)
            pk = rng.integers(0, 256, m * 64 + 64, dtype=np.uint8)
            starts = offsets.astype(np.int64) + self.data_off
        else:
            pk = rng.integers(0, 256, m * self.stride + (self.data_off and 64), dtype=np.uint8)
            starts = np.arange(m, dtype=np.int64) * self.stride + self.data_off
        starts = starts[:n]
        if keys is None:
            keys = make_keys(rng.integers(0, 1 << 32, m, dtype=np.uint64), rng.integers(0, 1 << 32, m, dtype=np.uint64),
                             rng.integers(0, 1 << 16, m), rng.integers(0, 1 << 16, m), rng.integers(0, 256, m))
        # packet 16a + b carries key (a + b) mod len: within 16 * len packets every key meets every header kind
        k = keys[(np.arange(n) // 16 + np.arange(n) % 16) % len(keys)]
        kind = np.array([KINDS.index(x) for x in KIND_PATTERN])[np.arange(n) % 16]
        is_ = lambda name: kind == KINDS.index(name)
        et = np.where(is_("et86dd"), 0x86DD, 0x0800)
        vihl = np.select([is_("ver6"), is_("ihl4"), is_("ihl6")], [0x65, 0x44, 0x46], 0x45)
        b20 = pk[starts + 20] & 0xC0                                        # the reserved bit and DF stay random
        b20 = np.where(is_("mf0"), b20 | 0x20, b20)
        b20 = np.where(is_("frag1") & (np.arange(n) % 32 >= 16), b20 | 0x1F, b20)   # offset 1 and offset 0x1F01
        pk[starts + 12], pk[starts + 13], pk[starts + 14] = et >> 8, et & 0xFF, vihl
        pk[starts + 20], pk[starts + 21] = b20, np.where(is_("frag1"), 1, 0)
        pk[starts + 23] = k["proto"]
        for j in range(4):
            pk[starts + 26 + j] = (k["src"] >> (24 - 8 * j)) & 0xFF
            pk[starts + 30 + j] = (k["dst"] >> (24 - 8 * j)) & 0xFF
        pk[starts + 34], pk[starts + 35] = k["sport"] >> 8, k["sport"] & 0xFF
        pk[starts + 36], pk[starts + 37] = k["dport"] >> 8, k["dport"] & 0xFF
        self.starts = starts
        self.inputs = {"pkts": pk}
        if self.imix:
            self.inputs["offsets"] = offsets
        # the restatement reads the bytes back
        self.skip, self.keys = keys_of(pk, starts)
        if n >= 16:
            assert seen_kinds(pk, starts) == set(KINDS), seen_kinds(pk, starts)
        plain = is_("plain") | is_("mf0")
        assert np.array_equal(self.keys[plain], k[plain])
        assert not self.keys["sport"][is_("frag1") | is_("ihl6")].any() and not self.keys["dport"][is_("frag1")].any()
        assert self.skip[is_("et86dd") | is_("ver6") | is_("ihl4")].all() and not self.skip[plain | is_("frag1")].any()
        fwd = np.ones(n, dtype=bool) if fwd is None else fwd
        ports = (np.arange(n) // 7) % K
        idx, counts, _ = tc.lay_lists(form, n, fwd, ports, K)
        self.inputs["idx"], self.inputs["counts"] = idx, counts
        words = lambda c: np.full((2 * PAD) // 4 + c, GUARD * 0x01010101, dtype=np.uint32)
        self.outs = [{"words": words(n), "out_idx": words(len(idx)), "out_count": words(len(counts)),
                      "status": words(4 * self.n_lists)}]
        self.expect = [{k_: v.copy() for k_, v in self.outs[0].items()}]

    # ---- the specification over this batch ----
    def words(self, rules) -> np.ndarray:
        return np.where(self.skip, np.uint32(SKIP), scan(rules, self.keys)).astype(np.uint32)

    def lists(self):
        """[(first word of the list in idx / out_idx, its entries as the clamps read them)]"""
        n, idx, cnt = self.n, self.inputs["idx"], self.inputs["counts"]
        if not n:
            return []
        if self.seg:
            return [(s * SEG, idx[s * SEG:s * SEG + min(int(cnt[s]), min(SEG, n - s * SEG))]) for s in range(len(cnt))]
        return [(q * n, idx[q * n:q * n + min(int(cnt[q]), n)]) for q in range(self.n_lists)]

    def want_classify(self, rules):
        self.expect[0]["words"][PAD // 4:PAD // 4 + self.n] = self.words(rules)

    def want_filter(self, rules, counters=None):
        """What the filter's outputs must hold; counters (n_rules u64, or None) get the hits added."""
        e, o, st, w = self.expect[0], PAD // 4, [], self.words(rules)
        for li, (first, ent) in enumerate(self.lists()):
            wi = w[np.minimum(ent.astype(np.int64), self.n - 1)]
            keep = (wi & DROP) == 0
            kept = ent[keep]
            e["out_idx"][o + first:o + first + len(kept)] = kept
            e["out_count"][o + li] = len(kept)
            st.append((len(kept), len(ent) - len(kept), int((wi == 0).sum()), int((wi == SKIP).sum())))
            if counters is not None:
                np.add.at(counters, (wi[(wi & HIT) != 0] & 0xFFFFFF).astype(np.int64), np.uint64(1))
        if self.n:
            if self.seg:
                st = [tuple(np.sum(st, axis=0))]
            for q, s4 in enumerate(st):
                e["status"][o + 4 * q:o + 4 * q + 4] = s4
        return e

    def status(self):
        return self.expect[0]["status"][PAD // 4:PAD // 4 + 4 * self.n_lists].reshape(-1, 4)

    # ---- descriptors ----
    def descs(self, addr_in, addr_out, with_results=True):
        """(Batch, AclDesc); addr_in(name) / addr_out(q, name) the base address of that array."""
        b = cg.Batch()
        if self.n:
            b.pkts, b.fwd_idx, b.fwd_count = addr_in("pkts"), addr_in("idx"), addr_in("counts")
        if self.imix:
            b.offsets = addr_in("offsets")
        b.n, b.stride, b.data_off = self.n, self.stride, self.data_off
        d = cg.AclDesc()
        if self.n:
            d.words, d.out_idx, d.out_count, d.status = (addr_out(0, k) + PAD for k in ("words", "out_idx", "out_count",
                                                                                       "status"))
        return b, d

    def check(self, got_of):
        for k, want in self.expect[0].items():
            got = got_of(0, k)
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                raise AssertionError(f"{k} ({self.form}, n={self.n}, {self.layout}): {len(bad)} words differ, first at "
                                     f"{bad[:6]} (guard {PAD // 4} words; got {got[bad[:6]]}, want {want[bad[:6]]})")
