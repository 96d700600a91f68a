"""Shared by test_lpm_live.py (host) and test_gpu_live_tables.py (device):
a model of the surviving rule set, and one crafted update script that puts
the patch kernel and the tbl8 group handling on their edges.

The expected state after any sequence of adds and deletes is an OracleLpm
built from the surviving rules alone (stop_at_error=False): the oracle has no
delete, so delete is pinned by the lookup function of the survivors.
"""
import numpy as np

import copgpu as cg
import oracle as orc

PATCH_SPAN = 1024        # cop_kernels.h COPK_PATCH_SPAN: entries per record after the host's cut
EINVAL, ENOSPC, ESTALE = -22, -28, -116


def mask(ip: int, depth: int) -> int:
    return ip & ((0xFFFFFFFF << (32 - depth)) & 0xFFFFFFFF) if depth else 0


class Model:
    """The rules a table holds, keyed by (masked ip, depth), next to the
    table itself: every operation goes to both, and the table's return code
    is checked against rte_lpm's rules worked out from the dict."""

    def __init__(self, table: cg.LpmTable, max_rules: int, number_tbl8s: int, rules=None):
        self.t, self.max_rules, self.tbl8s = table, max_rules, number_tbl8s
        self.held = {}
        self.ever = {}          # every (ip, depth) ever held: the probes' rule edges
        if rules is not None:
            r = table.rules()
            for ip, d, nh in zip(r["ip"].tolist(), r["depth"].tolist(), r["next_hop"].tolist()):
                self.held[(ip, d)] = nh
            self.ever.update(self.held)
        self.deep = {}          # /24 -> rules deeper than 24 it holds (its tbl8 group is in use)
        for ip, d in self.held:
            self._deep(ip, d, 1)

    def _deep(self, ip, d, by):
        if d > 24:
            self.deep[ip >> 8] = self.deep.get(ip >> 8, 0) + by
            if not self.deep[ip >> 8]:
                del self.deep[ip >> 8]

    def expect_add(self, ip, depth) -> int:
        if depth < 1 or depth > 32:
            return EINVAL
        key = (mask(ip, depth), depth)
        if key in self.held:
            return 0
        if len(self.held) >= self.max_rules:
            return ENOSPC
        if depth > 24 and (key[0] >> 8) not in self.deep and len(self.deep) >= self.tbl8s:
            return ENOSPC
        return 0

    def add(self, ip, depth, nh) -> int:
        want = self.expect_add(ip, depth)
        rc = self.t.add(ip, depth, nh)
        assert rc == want, (hex(ip), depth, rc, want)
        if rc == 0:
            key = (mask(ip, depth), depth)
            if key not in self.held:
                self._deep(key[0], depth, 1)
            self.held[key] = nh & 0x00FFFFFF
            self.ever[key] = 1
        return rc

    def delete(self, ip, depth) -> int:
        ok = 1 <= depth <= 32 and (mask(ip, depth), depth) in self.held
        rc = self.t.delete(ip, depth)
        assert rc == (0 if ok else EINVAL), (hex(ip), depth, rc)
        if rc == 0:
            del self.held[(mask(ip, depth), depth)]
            self._deep(mask(ip, depth), depth, -1)
        return rc

    def delete_all(self):
        assert self.t.delete_all() == 0
        self.held.clear()
        self.deep.clear()

    def run(self, ops):
        for op in ops:
            if op[0] == "add":
                self.add(*op[1:])
            elif op[0] == "del":
                self.delete(*op[1:])
            else:
                self.delete_all()

    def rules(self) -> np.ndarray:
        k = list(self.held)
        return cg.prefixes([ip for ip, _ in k], [d for _, d in k], [self.held[x] for x in k])

    def ever_rules(self) -> np.ndarray:
        k = list(self.ever)
        return cg.prefixes([ip for ip, _ in k], [d for _, d in k], [0] * len(k))

    def oracle(self) -> orc.OracleLpm:
        o = orc.OracleLpm(self.max_rules, self.tbl8s)
        r = self.rules()
        if len(r):
            first, err = o.setup(r["ip"], r["depth"], r["next_hop"], stop_at_error=False)
            assert first == -1, (first, err)   # the survivors were accepted one by one under the same limits
        return o


def ids_to_keys(ids: np.ndarray, rule_ip, rule_depth, id_of=None) -> np.ndarray:
    """Rule ids (-1: miss) as (ip << 8 | depth) keys (-1: miss), so that two
    tables with different id numbering compare by (prefix, depth). id_of: the
    ids the rule arrays are listed by (rules_ids()), default 0..n-1."""
    ids = np.asarray(ids, dtype=np.int64)
    key = (np.asarray(rule_ip, dtype=np.int64) << 8) | np.asarray(rule_depth, dtype=np.int64)
    n = int(max(int(np.max(id_of)) + 1 if id_of is not None and len(id_of) else len(key), 1))
    by_id = np.full(n + 1, -2, dtype=np.int64)
    if len(key):
        by_id[np.arange(len(key)) if id_of is None else np.asarray(id_of, dtype=np.int64)] = key
    out = np.where(ids < 0, -1, by_id[np.clip(ids, 0, n)])
    assert not (out == -2).any(), "a lookup returned a freed rule id"
    return out


# ---- the crafted update script ---------------------------------------------
# All of it lives in 10.0.0.0/9 (free of lpm_edges.filler() and of the crafted
# stride_edges rules, which sit in 11/8..13/8) except the steps that are about
# the ends of the address space and the action flips on 11.0.0.0/8.
def A(ip, depth, nh):
    return ("add", ip, depth, nh)


def D(ip, depth):
    return ("del", ip, depth)


def script():
    """A list of step groups; one update_* call follows each group."""
    g = []
    # a /32 into a plain /24 takes a group; deleting it releases the group
    g.append([A(0x0A010100, 24, 101), A(0x0A010107, 32, 102)])
    g.append([D(0x0A010107, 32)])
    # 256 distinct /32s fill one /24; every second one leaves
    g.append([A(0x0A020200 + o, 32, 0x200 + o) for o in range(256)])
    g.append([D(0x0A020200 + o, 32) for o in range(0, 256, 2)])
    # a /25 over a /24 holding /32s at offsets 1, 3, 5: runs of 1, 1, 1 and 122 entries at odd starts
    g.append([A(0x0A030300, 24, 301)] + [A(0x0A030300 + o, 32, 301 + o) for o in (1, 3, 5)])
    g.append([A(0x0A030300, 25, 310)])
    # a /13 over a nested /24 at entry offset 1: a tbl24 run from index 2 mod 4, 2046 long
    g.append([A(0x0A080100, 24, 401)])
    g.append([A(0x0A080000, 13, 402)])
    # a /12 (4096 entries) around /24s at offsets 1023, 2048, 3074: runs of
    # PATCH_SPAN - 1, PATCH_SPAN, PATCH_SPAN + 1 (and 1021) entries, the first from index 0,
    # the others from 0, 1 and 3 mod 4
    g.append([A(0x0A100000 + (o << 8), 24, 410 + i) for i, o in enumerate((PATCH_SPAN - 1, 2 * PATCH_SPAN,
                                                                       3 * PATCH_SPAN + 2))])
    g.append([A(0x0A100000, 12, 420)])
    # ... and with runs of 2047, 2048 and 2049 entries (two cuts each)
    g.append([A(0x0A200000 + (o << 8), 24, 430 + i) for i, o in enumerate((2047, 4096, 6146))])
    g.append([A(0x0A200000, 11, 440)])
    # the ends of the address space
    g.append([A(0x00000000, 1, 501)])
    g.append([D(0x00000000, 1)])
    g.append([A(0x00000000, 32, 502), A(0xFFFFFFFF, 32, 503)])
    # a rule with nested rules changes its action 0 -> 5 -> 0
    g.append([A(0x0B000000, 8, 5)])
    g.append([A(0x0B000000, 8, 0)])
    return g


def script_tail():
    """The whole table: delete_all, then ten rules again (the last group)."""
    return [[("del_all",)] + [A(0x0A400000 + (i << 12), 20 + i, 600 + i) for i in range(10)]]


def touched_addresses() -> np.ndarray:
    """Every address of every /24 the script's deep steps touch, and the
    entry boundaries of its tbl24 runs."""
    blocks = [0x0A010100, 0x0A020200, 0x0A030300, 0x0A080000, 0x0A080100, 0x0A080200, 0x00000000, 0xFFFFFF00]
    parts = [np.arange(b, b + 256, dtype=np.uint64) for b in blocks]
    for base, offs in ((0x0A100000, (PATCH_SPAN - 1, 2 * PATCH_SPAN, 3 * PATCH_SPAN + 2, 4095)),
                       (0x0A200000, (2047, 4096, 6146, 8191)), (0x0A080000, (0, 1, 2, 2047))):
        for o in offs:
            for e in (o - 1, o, o + 1):
                parts.append(np.array([base + (e << 8), base + (e << 8) + 255], dtype=np.uint64))
    return (np.unique(np.concatenate(parts)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
