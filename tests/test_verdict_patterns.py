"""The inputs of test_gpu_verdict_patterns.py are what they claim to be
(tests/verdict_patterns.py): for every pattern at every batch size the GPU
tests use, the oracle (fw_packet_handler, firewall.c:170-213; get_next_hop,
switch.c:93-136) run on the built frames gives exactly the prescribed
records, the numpy forward list and the prescribed counters; and the pattern
set reaches the edges it is there for (tiles of aggregate 0 and T, segment
lists of length 0..7, 255 and 256, a lone forward in lane 0 and in lane 63
of a wave, more than 256 silent tiles before a forwarding one). Conditions
on the inputs; the kernels are checked on the GPU."""
import functools

import numpy as np
import pytest

import copgpu as cg
import oracle as orc
import verdict_patterns as vp
from helpers import oracle_tables

S, F, L = vp.S, vp.F, vp.L


@functools.lru_cache(maxsize=None)
def oracle_twin():
    return oracle_tables(vp.fw_rules(), vp.route_rules(), fw_cfg=vp.FW_CFG)


def check(pk, n, rec, cnt, fwd, stages, n_ports, hits=None):
    fw, rt = oracle_twin()
    h = None if hits is None else np.zeros(fw.n_rules, np.uint64)
    ro, fo, co = orc.process(pk, n, rt=vp.routing_table(n_ports), n_ports=n_ports, stages=stages, fw=fw,
                             route=rt if stages & L else None, rule_hits=h)
    for f in ("verdict", "flags", "port", "route_nh"):
        bad = np.nonzero(ro[f] != rec[f])[0]
        assert bad.size == 0, f"{f} at {bad[:8]}: oracle {ro[f][bad[:8]]}, prescribed {rec[f][bad[:8]]}"
    assert np.array_equal(fo, vp.dense_list(fwd))
    assert co == cnt, (co, cnt)
    if hits is not None:
        assert np.array_equal(h, hits)


def test_tables_accept_every_rule_and_stay_small():
    for rules, cfg in ((vp.fw_rules(), vp.FW_CFG), (vp.route_rules(), (1 << 20, 1 << 16, False))):
        tab = cg.LpmTable(rules, *cfg)
        assert tab.report.n_failed == 0 and tab.report.n_distinct == len(rules)
        assert len(tab.intervals()[0]) < 64           # far below the LDS interval limit
        assert np.array_equal(tab.rules()["next_hop"], rules["next_hop"])     # rule id = position
    assert sorted(vp.FW_DROP_RULES + vp.FW_ACCEPT_RULES) == list(range(len(vp.FW_IP)))
    assert all(vp.FW_ACTION[r] != 0 for r in vp.FW_DROP_RULES) and all(vp.FW_ACTION[r] == 0 for r in vp.FW_ACCEPT_RULES)
    for K in (1, 5, 8):
        rt = vp.routing_table(K)
        assert [int(rt[k]) for k in vp.PORT_KEY] == list(range(8))
        assert rt[vp.NO_PORT_KEY] >= 8 and rt[vp.NO_PORT_KEY] != cg.UNKNOWN_PORT and rt[vp.UNKNOWN_KEY] == cg.UNKNOWN_PORT
        assert len({k >> 8 for k in vp.PORT_KEY}) == 8       # eight leaves of the device's two-level table


@pytest.mark.parametrize("n,T,names", vp.shapes())
def test_oracle_agrees_with_every_prescription(n, T, names):
    ports = np.arange(n) % 5
    for name, fwd in vp.select(n, T, names).items():
        cl = vp.classes_of(name, fwd)
        assert np.array_equal(vp.VERDICT_OF[cl] == cg.FORWARD, fwd), name
        pk, rec, cnt = vp.frames(cl, ports)
        assert cnt["forward"] == int(fwd.sum()) and cnt["rx"] == n
        check(pk, n, rec, cnt, fwd, S | F, 5, hits=vp.rule_hits(cl))
        if names is None and name in ("all", "even", "bern_63_64"):
            assert vp.rule_hits(cl)[vp.FW_ACCEPT_RULES].min() > 0, name     # every accept rule is hit
        if names is None and name in ("none", "odd", "bern_1_64"):
            assert vp.rule_hits(cl)[vp.FW_DROP_RULES].min() > 0, name       # and every drop rule


def test_single_class_batches_leave_eight_counters_zero():
    n = vp.ragged(256)
    for c in vp.DROP_CLASSES:
        name = f"none:{vp.CLASS_NAMES[c]}"
        cl = vp.classes_of(name, vp.patterns(n, 256)[name])
        assert (cl == c).all()
        cnt = vp.counters(cl)
        live = {k for k, v in cnt.items() if v}
        assert live == {"rx"} | {vp.DROP_FW: {"pkt_drop", "pkt_total"}, vp.PARSE_ETH: {"parse_err"},
                                 vp.PARSE_DST: {"parse_err"}, vp.NOT_IPV4: {"pkt_drop", "pkt_not_ipv4", "pkt_total"},
                                 vp.NO_PORT: {"no_port"}}[c]
    # the rotation keeps every counter alive in the mixed patterns
    cnt = vp.counters(vp.classes_of("odd", vp.patterns(n, 256)["odd"]))
    assert all(cnt[k] for k in cg.COUNTER_NAMES if k != "route_hit")


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8])
def test_oracle_agrees_with_every_port_layout(K):
    T = 1024
    n = vp.ragged(T)
    p = vp.patterns(n, T)
    for lname, ports in vp.port_layouts(n, T, K).items():
        assert ports.max() < K
        for mname in vp.DEMUX_MASKS:
            cl = vp.classes_of(mname, p[mname])
            pk, rec, cnt = vp.frames(cl, ports)
            check(pk, n, rec, cnt, p[mname], S | F, K)
            # the per-port lists partition the dense list, in order
            c, lists = vp.port_lists(p[mname], ports, K)
            assert np.array_equal(np.sort(np.concatenate(lists)), vp.dense_list(p[mname]))
            st = vp.port_stats(cl, ports, K)
            assert np.array_equal(st[:, 1], c) and st[:, 0].sum() == cnt["pkt_total"]


def test_oracle_agrees_with_port_layouts_on_the_long_chain():
    n, T, K = vp.LONG_N, 256, 8
    p = vp.patterns(n, T)
    for lname, ports in vp.port_layouts(n, T, K).items():
        for mname in ("all", "alt_tile_inv"):
            cl = vp.classes_of(mname, p[mname])
            pk, rec, cnt = vp.frames(cl, ports)
            check(pk, n, rec, cnt, p[mname], S | F, K)


def test_oracle_agrees_with_prescribed_route_hits():
    T = 1024
    n = vp.ragged(T)
    ports = np.arange(n) % 5
    for name, fwd in vp.select(n, T, vp.ROUTE_CASES).items():
        cl = vp.classes_of(name, fwd)
        rh = vp.route_hit_mask(n)
        pk, rec, cnt = vp.frames(cl, ports, route_hit=rh, stages=S | F | L)
        assert 0 < cnt["route_hit"] < cnt["pkt_total"] or cnt["pkt_total"] == 0
        assert set(np.unique(rec["route_nh"])) <= {0, *vp.ROUTE_NH}
        check(pk, n, rec, cnt, fwd, S | F | L, 5)


def test_pattern_set_hits_its_edges():
    seen = set()
    for T in (256, 1024, 2048):
        n = vp.ragged(T)
        assert n % 2 == 1 and n % 4 != 0 and n % vp.SEG == 3 and n // T >= 3
        p = vp.patterns(n, T)
        assert len(p) >= 36                               # (T = 256: positions 255 / T - 1 and 256 / T coincide)
        tile = np.arange(n) // T
        aggs = {int(m[tile == t].sum()) for m in p.values() for t in range(3)}
        assert {0, 1, T - 1, T} <= aggs, (T, sorted(aggs)[:4])
        seg_lens = {int(c) for m in p.values() for c in vp.seg_lists(m)[0]}
        assert {0, 1, 2, 3, 4, 5, 255, 256} <= seg_lens
        seen |= seg_lens
        # a wave whose only forward sits in lane 0, and one in lane 63
        lone = set()
        for m in p.values():
            w = m[:n // 64 * 64].reshape(-1, 64)
            for row in w[w.sum(axis=1) == 1]:
                lone.add(int(np.nonzero(row)[0][0]))
        assert {0, 63} <= lone, (T, sorted(lone))
        # every chunk residue of a tile's dense list and of its start
        assert {int(m[tile == 0].sum()) % 4 for m in p.values()} == {0, 1, 2, 3}
        assert [int(p["tile_head_k"][tile == t].sum()) for t in range(3)] == [2, 3, 4]
        # one_per_tile: tile t forwards its packet t alone
        assert list(np.nonzero(p["one_per_tile"])[0]) == [t * T + t for t in range(-(-n // T)) if t * T + t < n]
    assert set(range(8)) | {255, 256} <= seen             # 6 and 7 need the seventh segment (T >= 1024)
    # the long chain: 257 tiles publish aggregate 0 before the only forwarding one
    n, T = vp.LONG_N, 256
    p = vp.select(n, T, vp.LONG_CHAIN)
    tile = np.arange(n) // T
    assert tile[-1] == 257
    assert np.nonzero(p["last_tile_only"])[0].tolist() == [n - 1] and tile[n - 1] - 0 > 256
    assert p["first_tile_only"].sum() == 256 and not p["first_tile_only"][256:].any()
    per_tile = np.bincount(tile, weights=p["alt_tile_inv"])
    assert per_tile[257] == 1 and (per_tile[1:257:2] == 256).all() and (per_tile[0:257:2] == 0).all()
