"""Bulk-lookup words on the host (no GPU): cop_lpm_lookup_words is the exact
word cop_lookup_bulk returns, so it is checked here against the oracle
(rte_lpm_lookup: value and hit; the matching rule by (prefix, depth)), on the
tables that put the device lookups on their edges (tests/lpm_edges.py) and on
a table under live mutations; tests/c/lookup_words_replay.c repeats the latter
under sanitizers with a brute-force match; the audit report's layout and the
constants are compared with the header's.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import copgpu as cg
import lpm_edges as le
import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT, DROP = cg.LOOKUP_HIT, cg.LOOKUP_DROP
NH_MASK, RULE_MASK = 0x01FFFFFF, 0x05FFFFFF
EINVAL = -22
CFG_A = (4096, 64)
TABLES = ["crafted", "empty", "halves", "ends", "fw1k", "bkt_widths", "stride_edges", "routes100k"]


@functools.lru_cache(maxsize=None)
def rule_set(name):
    small = le.small_tables()
    if name in small:
        return small[name] + (None,)
    return {"bkt_widths": (le.bkt_widths(), le.RT_CFG, None),
            "stride_edges": (le.stride_edges(), le.RT_CFG, le.STRIDE_EXTRA),
            "routes100k": (le.routes100k(), le.RT_CFG, None)}[name]


def oracle_of(rules, cfg):
    o = orc.OracleLpm(max(cfg[0], len(rules), 1), cfg[1])
    if len(rules):
        o.setup(rules["ip"], rules["depth"], rules["next_hop"], stop_at_error=cfg[2])
    return o


def keys_of(ids, rule_ip, rule_depth, id_of=None):
    """Rule ids (-1: miss) as (ip << 8 | depth) keys (-1: miss): two tables
    that number their rules differently compare by (prefix, depth)."""
    ids = np.asarray(ids, dtype=np.int64)
    key = (np.asarray(rule_ip, dtype=np.int64) << 8) | np.asarray(rule_depth, dtype=np.int64)
    id_of = np.arange(len(key)) if id_of is None else np.asarray(id_of, dtype=np.int64)
    by_id = np.full(int(id_of.max()) + 2 if len(id_of) else 1, -2, dtype=np.int64)
    by_id[id_of] = key
    out = np.where(ids < 0, -1, by_id[np.clip(ids, 0, len(by_id) - 1)])
    assert not (out == -2).any(), "a word names a rule id the table does not hold"
    return out


def rule_word_parts(tab, words):
    """(matched rule as a (prefix, depth) key or -1, hit bit, drop bit) of RULE-form words."""
    r, ids = tab.rules_ids()
    hit = (words & HIT) != 0
    rid = np.where(hit, (words & 0x00FFFFFF).astype(np.int64), -1)
    return keys_of(rid, r["ip"], r["depth"], ids), hit, (words & DROP) != 0


@pytest.mark.parametrize("name", TABLES)
def test_words_against_the_oracle(name):
    rules, cfg, extra = rule_set(name)
    # next-hop form: the route table itself
    tab = le.table(rules, cfg)
    assert tab.report.n_failed == 0
    o = oracle_of(rules, cfg)
    p = le.boundary_probes(tab, extra)
    w = tab.lookup_words(p, cg.LOOKUP_NH)
    nh, hit = o.lookup(p)
    assert np.array_equal((w >> 24) & 1, hit)
    assert np.array_equal((w & 0x00FFFFFF)[hit == 1], (nh & 0x00FFFFFF)[hit == 1])
    assert not (w & ~np.uint32(NH_MASK)).any()
    assert not w[hit == 0].any()                        # a miss is exactly 0
    if name == "empty":
        assert not w.any()
    else:
        assert 0 < hit.sum()
    # rule-id form: the same prefixes as a firewall whose neighbours alternate
    # (fw1k: the generator's own actions)
    fr = rules if name == "fw1k" else le.fw_rules(rules)
    ft = le.table(fr, cfg)
    fo = oracle_of(fr, cfg)
    fw = ft.lookup_words(p, cg.LOOKUP_RULE)
    rid = ft.lookup_rules(p)
    r, ids = ft.rules_ids()
    action = np.zeros(int(ids.max()) + 1 if len(ids) else 1, dtype=np.uint32)
    action[ids] = r["next_hop"]
    safe = np.clip(rid, 0, None)
    want = np.where(rid >= 0, safe.astype(np.uint32) | np.uint32(HIT) | np.where(action[safe] != 0, DROP, 0).astype(np.uint32),
                    0).astype(np.uint32)
    assert np.array_equal(fw, want)
    assert not (fw & ~np.uint32(RULE_MASK)).any()
    assert not fw[rid < 0].any()
    # the matched rule, by (prefix, depth), is the oracle's
    oip, od, _ = fo.rules_by_id()
    assert np.array_equal(rule_word_parts(ft, fw)[0], keys_of(fo.match_rules(p), oip, od))
    if len(fr) > 1:
        d = (fw & DROP) != 0
        assert d.any() and (~d & ((fw & HIT) != 0)).any()        # both actions occur


def test_words_edge_arguments():
    rules, cfg, _ = rule_set("crafted")
    t = le.table(rules, cfg)
    L = cg.lib()
    ips = np.array([0x0B000000], np.uint32)
    out = np.full(1, 0xEEEEEEEE, np.uint32)
    assert L.cop_lpm_lookup_words(t.handle, cg.LOOKUP_NH, None, 0, None) == 0          # n = 0
    assert L.cop_lpm_lookup_words(t.handle, cg.LOOKUP_RULE, ips.ctypes.data, 0, out.ctypes.data) == 0
    assert out[0] == 0xEEEEEEEE
    for form in (2, -1, 7):
        assert L.cop_lpm_lookup_words(t.handle, form, ips.ctypes.data, 1, out.ctypes.data) == EINVAL
    assert L.cop_lpm_lookup_words(None, cg.LOOKUP_NH, ips.ctypes.data, 1, out.ctypes.data) == EINVAL
    assert L.cop_lpm_lookup_words(t.handle, cg.LOOKUP_NH, None, 1, out.ctypes.data) == EINVAL
    assert L.cop_lpm_lookup_words(t.handle, cg.LOOKUP_NH, ips.ctypes.data, 1, None) == EINVAL
    assert out[0] == 0xEEEEEEEE
    assert t.lookup_words(ips, cg.LOOKUP_NH)[0] & HIT


def mask(ip: int, depth: int) -> int:
    return ip & ((0xFFFFFFFF << (32 - depth)) & 0xFFFFFFFF)


def mutation_stream(seed, base_rules, n):
    """n mutations over a table holding base_rules (the shape of
    test_lpm_live.py's stream): adds of fresh rules, half of them nested in or
    around a held rule, next-hop overwrites (0 <-> non-zero among them) and
    deletes of held rules."""
    rng = np.random.default_rng(seed)
    held = {(int(r["ip"]), int(r["depth"])) for r in base_rules}
    order = list(held)
    out = []
    for _ in range(n):
        kind = rng.integers(0, 10)
        pick = order[int(rng.integers(0, len(order)))] if order else None
        if kind < 4 or pick is None:
            depth = int(rng.integers(1, 33))
            ip = int(rng.integers(0, 2**32))
            if pick is not None and rng.integers(0, 2):
                keep = min(depth, pick[1])
                ip = mask(pick[0], keep) | (ip & ~mask(0xFFFFFFFF, keep) & 0xFFFFFFFF)
            op = ("add", mask(ip, depth), depth, int(rng.integers(0, 1 << 24)))
        elif kind < 6:
            op = ("add", pick[0], pick[1], int(rng.integers(0, 3)))
        else:
            op = ("del", pick[0], pick[1])
        out.append(op)
        if op[0] == "add":
            if (op[1], op[2]) not in held:
                held.add((op[1], op[2]))
                order.append((op[1], op[2]))
        else:
            held.discard((op[1], op[2]))
            order.remove((op[1], op[2]))
    return out


def base_2000():
    return cg.gen_rules(0xB0CA, 2000, cg.GEN_FW, 40)


def test_words_after_live_mutations():
    """1,000 mutations on a 2,000-rule table: every 100, both forms' words
    equal those of a table rebuilt from the survivors (rule ids differ once a
    rule was deleted: the RULE words compare by (prefix, depth) and flags)."""
    rules = base_2000()
    t = cg.LpmTable(rules, CFG_A[0], CFG_A[1], False)
    ops = mutation_stream(0x10CA, t.rules(), 1000)
    ever = [t.rules()]
    applied = 0
    for i, op in enumerate(ops):
        rc = t.add(*op[1:]) if op[0] == "add" else t.delete(*op[1:])
        applied += rc == 0
        if op[0] == "add":
            ever.append(cg.prefixes([op[1]], [op[2]], [op[3]]))
        if (i + 1) % 100:
            continue
        surv = t.rules()
        fresh = cg.LpmTable(surv, CFG_A[0], CFG_A[1], False)
        assert len(fresh.rules()) == len(surv)
        p = np.union1d(le.boundary_probes(np.concatenate(ever)), t.audit_probes(cg.LOOKUP_RULE))
        assert np.array_equal(t.lookup_words(p, cg.LOOKUP_NH), fresh.lookup_words(p, cg.LOOKUP_NH))
        a, b = t.lookup_words(p, cg.LOOKUP_RULE), fresh.lookup_words(p, cg.LOOKUP_RULE)
        for x, y in zip(rule_word_parts(t, a), rule_word_parts(fresh, b)):
            assert np.array_equal(x, y)
        # and the oracle of the survivors
        nh, hit = oracle_of(surv, (CFG_A[0], CFG_A[1], False)).lookup(p)
        w = t.lookup_words(p, cg.LOOKUP_NH)
        assert np.array_equal((w >> 24) & 1, hit) and np.array_equal((w & 0xFFFFFF)[hit == 1], nh[hit == 1] & 0xFFFFFF)
    assert applied > 900 and t.generation == applied
    assert not np.array_equal(t.rules_ids()[1], np.arange(len(t.rules())))     # ids were freed and reused


def test_audit_probe_set():
    """For every interval start s of the form: s and s - 1, plus 0xFFFFFFFF;
    ascending, no repeats."""
    for name in ("empty", "ends", "halves", "crafted", "fw1k"):
        rules, cfg, _ = rule_set(name)
        t = le.table(rules, cfg)
        s, _ = t.intervals()
        p = t.audit_probes(cg.LOOKUP_NH)
        s64 = s.astype(np.int64)
        want = np.unique(np.concatenate([s64, s64[s64 > 0] - 1, [0xFFFFFFFF]])).astype(np.uint32)
        assert np.array_equal(p, want), name
        assert len(p) <= 2 * len(s) + 1
        # the rule-id form keeps at least the next-hop form's boundaries (where
        # the next hop changes, the matching rule does)
        q = t.audit_probes(cg.LOOKUP_RULE)
        assert (np.diff(q.astype(np.int64)) > 0).all() and q[0] == 0 and q[-1] == 0xFFFFFFFF
        assert np.isin(p, q).all(), name


def test_host_table_under_sanitizers(tmp_path):
    """tests/c/lookup_words_replay.c, a stand-alone program: lpm_build.c,
    lpm_live.c and lpm_lookup.c built with -fsanitize=address,undefined, the
    words and the audit's probe set against a brute-force longest-prefix
    match over a mutation stream."""
    rules = base_2000()
    t = cg.LpmTable(rules, CFG_A[0], CFG_A[1], False)
    ops = mutation_stream(0x10CA, t.rules(), 1000)
    stream = tmp_path / "stream.txt"
    with open(stream, "w") as f:
        f.write(f"{CFG_A[0]} {CFG_A[1]} {len(rules)} {len(ops)}\n")
        for r in rules:
            f.write(f"{int(r['ip'])} {int(r['depth'])} {int(r['next_hop'])}\n")
        for op in ops:
            f.write(f"A {op[1]} {op[2]} {op[3]}\n" if op[0] == "add" else f"D {op[1]} {op[2]} 0\n")
    exe = tmp_path / "lookup_words_replay"
    csrc = os.path.join(ROOT, "ghost-dataplane_amd", "csrc")
    cc = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", csrc,
                         os.path.join(ROOT, "tests", "c", "lookup_words_replay.c"), os.path.join(csrc, "lpm_build.c"),
                         os.path.join(csrc, "lpm_live.c"), os.path.join(csrc, "lpm_lookup.c"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe), str(stream)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "replayed 1000 mutations" in run.stdout
    for op in ops:
        t.add(*op[1:]) if op[0] == "add" else t.delete(*op[1:])
    assert f"held {len(t.rules())} generation {t.generation}" in run.stdout


def test_audit_report_layout_and_constants_match_c(tmp_path):
    """cg.AuditReport mirrors cop_audit_report field for field, and the
    binding's constants are the header's."""
    consts = {"COP_LOOKUP_HIT": cg.LOOKUP_HIT, "COP_LOOKUP_DROP": cg.LOOKUP_DROP, "COP_LOOKUP_NH": cg.LOOKUP_NH,
              "COP_LOOKUP_RULE": cg.LOOKUP_RULE, "COP_STAGE_FW": cg.STAGE_FW, "COP_STAGE_LPM": cg.STAGE_LPM}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cop_gpu.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(cop_audit_report));']
    for f, _ in cg.AuditReport._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(cop_audit_report, {f}));')
    for c in consts:
        lines.append(f'printf("{c} %llu\\n", (unsigned long long)({c}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[::2], map(int, out[1::2])))
    assert got["size"] == ctypes.sizeof(cg.AuditReport)
    for f, _ in cg.AuditReport._fields_:
        assert got[f] == getattr(cg.AuditReport, f).offset, f
    for c, v in consts.items():
        assert got[c] == v, c
    assert cg.LOOKUP_HIT == 0x01000000          # RTE_LPM_LOOKUP_SUCCESS
    # the internal header's staging chunk is the binding's
    internal = open(os.path.join(ROOT, "ghost-dataplane_amd", "csrc", "cop_internal.h")).read()
    assert "#define COP_LOOKUP_STAGE_WORDS (1u << 20)" in internal and cg.LOOKUP_STAGE_WORDS == 1 << 20
