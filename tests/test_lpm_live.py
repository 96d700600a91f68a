"""Live LPM tables on the host (no GPU): cop_lpm_add / cop_lpm_delete /
cop_lpm_delete_all keep every derived form of the table equal to a rebuild,
return rte_lpm's codes, hand out rule ids as documented, and journal their
changes; cop_lpm_patch_records turns the journal into disjoint fill records
that bring a painted DIR-24-8 image to the same lookups as a fresh paint.

The expected state is always an OracleLpm built from the surviving rules
(live_tables.Model); a table built by cop_lpm_build from the same survivors
is the second opinion for the exact interval arrays.
"""
import os
import subprocess

import numpy as np
import pytest

import copgpu as cg
import lpm_edges as le
import oracle as orc
from live_tables import EINVAL, ENOSPC, ESTALE, Model, ids_to_keys, mask, script, script_tail, touched_addresses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_A = (4096, 64)


def dir_lookup(t24, t8, ips):
    e = t24[ips >> 8]
    ext = (e & 0x03000000) == 0x03000000
    e = e.copy()
    e[ext] = t8[(e[ext] & 0x00FFFFFF).astype(np.int64) * 256 + (ips[ext] & 0xFF)]
    return e & 0x00FFFFFF, ((e >> 24) & 1).astype(np.uint8)


def check_against_rebuild(m: Model, probes: np.ndarray):
    """Every derived form of m.t against the oracle (and a rebuilt table) of
    the surviving rules."""
    t, o = m.t, m.oracle()
    nh, hit = o.lookup(probes)
    # intervals(): the lookups, and the arrays themselves against a rebuild
    inh, ihit = le.interval_search(t, probes)
    assert np.array_equal(inh, nh) and np.array_equal(ihit, hit)
    surv = m.rules()
    fresh = cg.LpmTable(surv, m.max_rules, m.tbl8s, False)
    for a, b in zip(t.intervals(), fresh.intervals()):
        assert np.array_equal(a, b)
    # export_dir24 (n_ext and the paint)
    t24, t8 = t.dir24()
    f24, f8 = fresh.dir24()
    assert len(t8) == len(f8)
    dnh, dhit = dir_lookup(t24, t8, probes)
    assert np.array_equal(dnh, nh) and np.array_equal(dhit, hit)
    # lookup_rules, by (prefix, depth): ids differ from the oracle's once a rule was deleted
    r, ids = t.rules_ids()
    got = ids_to_keys(t.lookup_rules(probes), r["ip"], r["depth"], ids)
    oip, od, _ = o.rules_by_id()
    assert np.array_equal(got, ids_to_keys(o.match_rules(probes), oip, od))
    # a second opinion on the lookups
    bnh, bhit = orc.brute_lookup(surv["ip"], surv["depth"], surv["next_hop"], probes[:4096])
    assert np.array_equal(bnh, nh[:4096]) and np.array_equal(bhit, hit[:4096])
    # the report
    assert t.report.tbl8_used == o.tbl8_used == fresh.report.tbl8_used
    assert t.report.n_distinct == o.n_rules == len(surv)
    assert t.report.n_intervals == fresh.report.n_intervals


def mutation_stream(seed, base_rules, n):
    """n mutations over a table holding base_rules: adds of fresh rules
    (half of them nested in or around a held rule), next-hop overwrites and
    deletes of held rules. Yields ("add", ip, depth, nh) / ("del", ip, depth),
    chosen against the evolving set, so every delete names a held rule."""
    rng = np.random.default_rng(seed)
    held = {(int(r["ip"]), int(r["depth"])) for r in base_rules}
    order = list(held)
    out = []
    for _ in range(n):
        kind = rng.integers(0, 10)
        pick = order[int(rng.integers(0, len(order)))] if order else None
        if kind < 4 or pick is None:            # a fresh rule
            depth = int(rng.integers(1, 33))
            ip = int(rng.integers(0, 2**32))
            if pick is not None and rng.integers(0, 2):
                # share the top bits of a held rule: nests in it, or covers it
                keep = min(depth, pick[1])
                ip = (pick[0] & mask(0xFFFFFFFF, keep)) | (ip & ~mask(0xFFFFFFFF, keep) & 0xFFFFFFFF)
            op = ("add", mask(ip, depth), depth, int(rng.integers(0, 1 << 24)))
        elif kind < 6:                          # overwrite (sometimes 0 <-> non-zero)
            op = ("add", pick[0], pick[1], int(rng.integers(0, 3)))
        else:
            op = ("del", pick[0], pick[1])
        out.append(op)
        if op[0] == "add":
            # (an add the table refuses is retried by the stream as "held": harmless, it is
            # then a delete of an absent rule at worst; apply() below keeps the truth)
            if (op[1], op[2]) not in held:
                held.add((op[1], op[2]))
                order.append((op[1], op[2]))
        else:
            held.discard((op[1], op[2]))
            order.remove((op[1], op[2]))
    return out


def base_2000():
    return cg.gen_rules(0xA11CE, 2000, cg.GEN_FW, 40)


def test_random_mutations_equal_a_rebuild():
    rules = base_2000()
    t = cg.LpmTable(rules, CFG_A[0], CFG_A[1], False)
    m = Model(t, *CFG_A, rules=rules)
    ops = mutation_stream(0x11FE, t.rules(), 2000)
    for i, op in enumerate(ops):
        g = t.generation
        if op[0] == "add":
            rc = t.add(*op[1:])
            assert rc == m.expect_add(op[1], op[2]), op
            if rc == 0:
                # (through the model's own book-keeping, without a second table call)
                key = (op[1], op[2])
                if key not in m.held:
                    m._deep(op[1], op[2], 1)
                m.held[key] = op[3] & 0x00FFFFFF
                m.ever[key] = 1
        else:
            present = (op[1], op[2]) in m.held
            rc = t.delete(*op[1:])
            assert rc == (0 if present else EINVAL), op
            if rc == 0:
                del m.held[(op[1], op[2])]
                m._deep(op[1], op[2], -1)
        assert t.generation == g + (1 if rc == 0 else 0)
        if (i + 1) % 100 == 0:
            check_against_rebuild(m, le.boundary_probes(m.ever_rules()))
    assert len(m.ever) > len(rules) + 300 and len(m.held) != len(rules)


def test_return_codes_and_unchanged_after_failure():
    t = cg.LpmTable.empty(8, 2)
    m = Model(t, 8, 2)
    probes = np.array([0, 0x0A000000, 0x0A000001, 0x0A0000FF, 0x0A000100, 0x0B000001, 0xFFFFFFFF], np.uint32)

    def unchanged(f, want):
        g, before = t.generation, [a.copy() for a in t.intervals()]
        assert f() == want
        assert t.generation == g
        for a, b in zip(t.intervals(), before):
            assert np.array_equal(a, b)

    m.add(0x0A000000, 8, 1)
    unchanged(lambda: t.delete(0x0B000000, 8), EINVAL)        # not held: DPDK's -EINVAL, not -ENOENT
    unchanged(lambda: t.delete(0x0A000000, 9), EINVAL)        # held at another depth only
    unchanged(lambda: t.delete(0x0A000000, 0), EINVAL)
    unchanged(lambda: t.delete(0x0A000000, 33), EINVAL)
    unchanged(lambda: t.add(0x0A000000, 0, 1), EINVAL)
    unchanged(lambda: t.add(0x0A000000, 33, 1), EINVAL)
    assert t.is_rule_present(0x0A123456, 8) == (1, 1)          # the address is masked to the depth
    assert t.is_rule_present(0x0A000000, 9) == (0, None)
    assert t.is_rule_present(0x0A000000, 0)[0] == EINVAL and t.is_rule_present(0x0A000000, 33)[0] == EINVAL
    # the last tbl8 group: two /24s hold deep rules, a third cannot
    m.add(0x0A000001, 32, 2)
    m.add(0x0A000080, 25, 3)                                   # same /24: same group
    m.add(0x0A000101, 32, 4)
    assert t.report.tbl8_used == 2
    unchanged(lambda: t.add(0x0A000201, 32, 5), ENOSPC)
    m.delete(0x0A000101, 32)                                   # the /24's last deep rule: the group is free again
    assert t.report.tbl8_used == 1
    m.add(0x0A000201, 32, 5)
    check_against_rebuild(m, np.concatenate([probes, le.boundary_probes(m.ever_rules())]))
    # max_rules: 4 held now, 8 allowed; an overwrite still succeeds at the limit
    for i in range(4):
        m.add(0x0C000000 + (i << 16), 16, 10 + i)
    unchanged(lambda: t.add(0x0D000000, 8, 9), ENOSPC)
    m.add(0x0C000000, 16, 99)
    m.delete(0x0C000000, 16)
    m.add(0x0D000000, 8, 9)
    check_against_rebuild(m, le.boundary_probes(m.ever_rules()))
    # a built table answers is_rule_present before its first mutation too
    b = cg.LpmTable(m.rules(), 8, 2, False)
    assert b.is_rule_present(0x0D000000, 8) == (1, 9) and b.is_rule_present(0x0D000000, 9) == (0, None)
    # delete_all
    m.delete_all()
    assert t.report.n_distinct == 0 and t.report.tbl8_used == 0 and len(t.rules()) == 0
    s, v = t.intervals()
    assert s.tolist() == [0] and v.tolist() == [0]
    m.add(0x0A000001, 32, 7)
    check_against_rebuild(m, le.boundary_probes(m.ever_rules()))


def test_rule_ids():
    rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    built = cg.LpmTable(rules, 1024, 24, True)
    # a table filled by add() alone numbers its rules as cop_lpm_build does
    t = cg.LpmTable.empty(1024, 24)
    for r in rules:
        if t.add(int(r["ip"]), int(r["depth"]), int(r["next_hop"])) != 0:
            break                                  # stop at the first error, as the build above
    br, bi = built.rules_ids()
    tr, ti = t.rules_ids()
    assert np.array_equal(bi, np.arange(len(br))) and np.array_equal(ti, bi)
    assert np.array_equal(tr, br) and np.array_equal(t.rules(), built.rules())
    # deleting ids 3 and 7 moves no other id; rules() skips the holes
    for tab in (t, built):
        r0, i0 = tab.rules_ids()
        for k in (3, 7):
            assert tab.delete(int(r0["ip"][k]), int(r0["depth"][k])) == 0
        r1, i1 = tab.rules_ids()
        keep = np.ones(len(r0), bool)
        keep[[3, 7]] = False
        assert np.array_equal(i1, i0[keep]) and np.array_equal(r1, r0[keep])
        assert np.array_equal(tab.rules(), r0[keep])
        probes = le.boundary_probes(r0)
        assert not np.isin(tab.lookup_rules(probes), [3, 7]).any()
        # the next two new rules take 3, then 7, then the id space grows
        assert tab.add(0xC6336400, 24, 1) == 0 and tab.add(0xC6336500, 24, 1) == 0
        assert tab.add(0xC6336600, 24, 1) == 0
        r2, i2 = tab.rules_ids()
        by = {(int(a), int(d)): int(i) for a, d, i in zip(r2["ip"], r2["depth"], i2)}
        assert by[(0xC6336400, 24)] == 3 and by[(0xC6336500, 24)] == 7 and by[(0xC6336600, 24)] == len(r0)
        assert tab.lookup_rules(np.array([0xC6336401, 0xC6336501], np.uint32)).tolist() == [3, 7]


def crafted_table():
    rules = le.stride_edges_crafted()
    return rules, cg.LpmTable(rules, 1 << 20, 1 << 16, False)


@pytest.mark.parametrize("form", [le.FORM_NH, le.FORM_RULE], ids=["nh", "rule"])
def test_patch_records_against_a_fresh_paint(form):
    rules, t = crafted_table()
    if form == le.FORM_RULE:
        rules = le.fw_rules(rules)
        t = cg.LpmTable(rules, 1 << 20, 1 << 16, False)
    m = Model(t, 1 << 20, 1 << 16, rules=rules)
    img = t.live_image(form, cap_groups=64)
    extra = touched_addresses()
    for group in script() + script_tail():
        m.run(group)
        recs, rep = img.records()
        assert recs is not None, rep
        assert rep["n_changes"] == len(group) and rep["n_records"] == len(recs)
        # disjoint: no entry of either table is written twice
        for tb in (0, 1):
            r = recs[recs["table"] == tb]
            r = r[np.argsort(r["first"], kind="stable")]
            assert (r["count"] > 0).all()
            assert (r["first"][1:].astype(np.int64) >= r["first"][:-1].astype(np.int64) + r["count"][:-1]).all()
            assert int(r["count"].sum()) == rep["tbl8_entries" if tb else "tbl24_entries"]
        img.apply(recs)
        fresh = t.live_image(form)
        probes = np.unique(np.concatenate([le.boundary_probes(m.ever_rules()), extra]))
        assert np.array_equal(img.lookup(probes), fresh.lookup(probes))
        # the RULE form's entries carry ids, the NH form's next hops: either way the oracle agrees
        o = m.oracle()
        nh, hit = o.lookup(probes)
        e = img.lookup(probes)
        assert np.array_equal((e >> 24) & 1, hit)
        if form == le.FORM_NH:
            assert np.array_equal(e & 0x00FFFFFF, nh)
    # every group was released again by delete_all
    assert rep["groups_released"] > 0


def test_patch_entry_counts_on_an_empty_table():
    for ip, depth, want in ((0x0A010100, 24, 1), (0x0A080000, 13, 2048), (0x80000000, 1, 1 << 23)):
        t = cg.LpmTable.empty(16, 4)
        img = t.live_image(le.FORM_NH, cap_groups=4)
        assert t.add(ip, depth, 9) == 0
        recs, rep = img.records()
        assert rep["tbl24_entries"] == want and rep["tbl8_entries"] == 0 and rep["groups_taken"] == 0
        assert len(recs) == 1 and recs[0]["first"] == ip >> 8 and recs[0]["count"] == want
        assert recs[0]["entry"] & 0x01FFFFFF == 0x01000009
    # a /32 takes a group and paints all of it: 256 tbl8 entries, one tbl24 entry
    t = cg.LpmTable.empty(16, 4)
    img = t.live_image(le.FORM_NH, cap_groups=4)
    assert t.add(0x0A010107, 32, 9) == 0
    recs, rep = img.records()
    assert (rep["tbl24_entries"], rep["tbl8_entries"], rep["groups_taken"]) == (1, 256, 1)
    # a second /32 beside it: its own entry alone
    assert t.add(0x0A010109, 32, 8) == 0
    recs, rep = img.records()
    assert (rep["tbl24_entries"], rep["tbl8_entries"], rep["groups_taken"]) == (0, 1, 0)
    # out of groups: the caller repaints
    t2 = cg.LpmTable.empty(16, 4)
    img2 = t2.live_image(le.FORM_NH, cap_groups=1)
    assert t2.add(0x0A010107, 32, 9) == 0 and t2.add(0x0A010207, 32, 9) == 0
    assert img2.records() == (None, ENOSPC)


def test_journal_overflow_reports_too_old():
    t = cg.LpmTable.empty(64, 4)
    img = t.live_image(le.FORM_NH, cap_groups=4)
    t.journal_set_cap(8)
    for i in range(8):
        assert t.add(0x0A000000 + (i << 8), 24, i + 1) == 0
    recs, rep = img.records()                    # eight changes: the journal still reaches back
    assert rep["n_changes"] == 8 and len(recs) == 8
    img.apply(recs)
    old = t.live_image(le.FORM_NH, cap_groups=4)
    for i in range(9):
        assert t.add(0x0B000000 + (i << 8), 24, i + 1) == 0
    assert old.records() == (None, ESTALE)       # nine changes, eight journalled: too old
    assert old.records() == (None, ESTALE)       # and it stays so
    fresh = t.live_image(le.FORM_NH, cap_groups=4)
    assert fresh.records()[1]["n_changes"] == 0  # a new image starts at the current generation


def test_update_report_layout_matches_c(tmp_path):
    """cg.UpdateReport mirrors cop_update_report field for field."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cop_gpu.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(cop_update_report));']
    for f, _ in cg.UpdateReport._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(cop_update_report, {f}));')
    lines.append("return COP_CFG_LIVE_TABLES == 0x400u ? 0 : 1;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[::2], map(int, out[1::2])))
    import ctypes
    assert got["size"] == ctypes.sizeof(cg.UpdateReport)
    for f, _ in cg.UpdateReport._fields_:
        assert got[f] == getattr(cg.UpdateReport, f).offset, f
    assert cg.CFG_LIVE_TABLES == 0x400


def test_host_table_under_sanitizers(tmp_path):
    """tests/c/lpm_live_replay.c, a stand-alone program, replays test (a)'s
    mutation stream on lpm_build.c + lpm_live.c built with
    -fsanitize=address,undefined, checks lookups against a brute-force
    longest-prefix match of the survivors, and builds patch records."""
    rules = base_2000()
    t = cg.LpmTable(rules, CFG_A[0], CFG_A[1], False)
    ops = mutation_stream(0x11FE, t.rules(), 2000)
    stream = tmp_path / "stream.txt"
    with open(stream, "w") as f:
        f.write(f"{CFG_A[0]} {CFG_A[1]} {len(rules)} {len(ops)}\n")
        for r in rules:
            f.write(f"{int(r['ip'])} {int(r['depth'])} {int(r['next_hop'])}\n")
        for op in ops:
            f.write(f"A {op[1]} {op[2]} {op[3]}\n" if op[0] == "add" else f"D {op[1]} {op[2]} 0\n")
    exe = tmp_path / "lpm_live_replay"
    csrc = os.path.join(ROOT, "ghost-dataplane_amd", "csrc")
    cc = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", csrc,
                         os.path.join(ROOT, "tests", "c", "lpm_live_replay.c"), os.path.join(csrc, "lpm_build.c"),
                         os.path.join(csrc, "lpm_live.c"), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe), str(stream)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "replayed 2000 mutations" in run.stdout
    # the program's final state is this binding's
    for op in ops:
        t.add(*op[1:]) if op[0] == "add" else t.delete(*op[1:])
    assert f"held {len(t.rules())} generation {t.generation}" in run.stdout
