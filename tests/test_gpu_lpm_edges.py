"""GPU: every device LPM lookup at every prefix boundary.

The seven device lookups of csrc/cop_device.h (ivt_value / ivt_search in
LDS, tbl8_step and tbl8_issue / tbl8_finish over plain and packed DIR-24-8
groups, trie_walk, bkt_step and bkt_pairs_issue / bkt_pairs_finish) are each
run over the first and last address of every rule of tables built to put them
on their edges (tests/lpm_edges.py; their structure is checked on the host in
test_lpm_edges.py), the address either side of each and the two ends of the
address space, as firewall sources and route destinations of one batch.
Every record field and the forward list must equal the oracle's
(rte_lpm_lookup, firewall.c:194; fw_packet_handler, firewall.c:170-213), bit
for bit, through the one-shot kernel at each tile size, the poll-mode step
path, and the poll-mode engine bench.py times.
"""
import functools

import numpy as np
import pytest

import copgpu as cg
import lpm_edges as le
import oracle as orc
from helpers import assert_parity, gpu_run
from test_gpu_seg import nseg, seg_to_dense
from test_gpu_tables import MODES, ROUTE_FORM

pytestmark = pytest.mark.gpu

S, F, L = cg.STAGE_PARSE, cg.STAGE_FW, cg.STAGE_LPM
LARGE = ("bkt_widths", "stride_edges")
FW_LARGE = ("forced", "packed", "fwbkt")     # modes whose firewall table leaves LDS too
NO_PCT = dict(pct_non_ipv4=0, pct_bad_version=0, pct_unknown_dst=0)


@functools.lru_cache(maxsize=None)
def rule_set(name):
    """name -> (rules, LpmTable configuration, extra probes)."""
    small = le.small_tables()
    if name in small:
        return small[name] + (None,)
    if name == "bkt_widths":
        return le.bkt_widths(), le.RT_CFG, None
    if name == "stride_edges":
        return le.stride_edges(), le.RT_CFG, le.STRIDE_EXTRA
    if name == "routes100k":
        return le.routes100k(), le.RT_CFG, None
    assert name.startswith("lds_limit"), name
    return le.lds_limit(int(name[9:])), le.RT_CFG, None


@functools.lru_cache(maxsize=None)
def tables(name, fw):
    """(LpmTable, oracle table, boundary probes) of rule set `name`, as the
    route table or (fw) as a firewall whose neighbouring rules alternate."""
    rules, cfg, extra = rule_set(name)
    if fw:
        rules = le.fw_rules(rules)
    tab = le.table(rules, cfg)
    assert tab.report.n_failed == 0, tab.report.as_dict()
    o = orc.OracleLpm(max(cfg[0], len(rules), 1), cfg[1])
    if len(rules):
        o.setup(rules["ip"], rules["depth"], rules["next_hop"], stop_at_error=cfg[2])
    return tab, o, le.boundary_probes(tab, extra)


@functools.lru_cache(maxsize=None)
def probe_set(route, fw, multiple=1):
    """Both tables' boundary probes (at most 200k, then repeated up to a
    multiple of `multiple`): sources ascending, destinations descending."""
    p = np.union1d(tables(route, False)[2], tables(fw, True)[2])
    p = le.pad_to(le.subsample(p), multiple)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def batch(route, fw, stages, multiple=1):
    """(frames, n, oracle records, oracle forward list): computed once."""
    p = probe_set(route, fw, multiple)
    pk = le.probe_frames(p)
    ro, fo, _ = orc.process(pk, len(p), stages=stages, fw=tables(fw, True)[1], route=tables(route, False)[1])
    for a in (pk, ro, fo):
        a.setflags(write=False)
    return pk, len(p), ro, fo


def load(ctx, route, fw):
    ctx.set_fw_table(tables(fw, True)[0])
    ctx.set_route_lpm(tables(route, False)[0])


ONESHOT = [(t, m, p) for t in LARGE for m in MODES for p in (1, 4, 8)
           if p < 8 or m in ("auto", "forced", "packed", "trie")]    # the bucketed forms run at most 4 per lane


@pytest.mark.parametrize("route,mode,ppt", ONESHOT)
def test_oneshot_boundaries_large_tables(gpu_ctx_factory, monkeypatch, route, mode, ppt):
    """The one-shot kernel at 1, 4 and 8 packets per lane ($COP_PPT) over the
    whole probe batch, no parse stage (every probe reaches both lookups):
    tbl8_step plain and packed, trie_walk and bkt_step for the route stage;
    the firewall in LDS (ivt_value), or the same large table keyed by rule
    id in DIR-24-8 / bucketed form."""
    monkeypatch.setenv("COP_TBL8", MODES[mode][1])
    monkeypatch.setenv("COP_PPT", str(ppt))
    fw = route if mode in FW_LARGE else "crafted"
    ctx = gpu_ctx_factory(stages=F | L, flags=MODES[mode][0])
    load(ctx, route, fw)
    assert ctx.route_form() == ROUTE_FORM.get(mode, "dir")
    pk, n, ro, fo = batch(route, fw, F | L)
    assert 150000 < n <= 200000
    assert 0.3 < (ro["flags"] & 1).mean() < 1            # route hits and misses
    assert 100 < (ro["verdict"] == cg.DROP_FW).sum() < len(fo)   # both firewall actions
    if fw == route:
        assert 0.3 < (ro["verdict"] == cg.DROP_FW).mean() < 0.7
    rg, fg, _ = gpu_run(ctx, pk, n, batches=1)
    assert_parity(rg, fg, ro, fo)


@pytest.mark.parametrize("name", ["crafted", "empty", "halves", "ends", "fw1k", "routes100k", "lds_limit4096"])
def test_oneshot_boundaries_small_tables(gpu_ctx_factory, monkeypatch, name):
    """Firewall and route stage both from one table with the default mode
    selection: the LDS interval form (u16 bucket index, 0xFFFFFFFF pads,
    lift levels from the widest bucket) for the small ones, among them the
    empty table, ip 0 and ip 0xFFFFFFFF as interval starts, and 8192
    intervals in each table, the LDS limit (where the launch may move one of
    the two to DIR-24-8: the records are the same)."""
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.delenv("COP_TBL8", raising=False)
    ctx = gpu_ctx_factory(stages=F | L)
    load(ctx, name, name)
    if name != "lds_limit4096":
        assert ctx.route_form() == ("dir" if name == "routes100k" else "lds")
    pk, n, ro, fo = batch(name, name, F | L)
    rg, fg, _ = gpu_run(ctx, pk, n, batches=1)
    assert_parity(rg, fg, ro, fo)


def test_one_interval_past_the_lds_limit(gpu_ctx_factory, monkeypatch):
    """8194 intervals: the route table must leave LDS."""
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.delenv("COP_TBL8", raising=False)
    ctx = gpu_ctx_factory(stages=F | L)
    load(ctx, "lds_limit4097", "crafted")
    assert ctx.route_form() == "dir"
    pk, n, ro, fo = batch("lds_limit4097", "crafted", F | L)
    rg, fg, _ = gpu_run(ctx, pk, n, batches=1)
    assert_parity(rg, fg, ro, fo)


@pytest.mark.parametrize("mode", ["bkt", "trie"])
def test_boundaries_beside_dead_lanes(gpu_ctx_factory, monkeypatch, mode):
    """With the parse stage on, the default routing table drops about 5 % of
    the probe frames before the lookups: probing lanes sit beside masked
    lanes in one wave (the wave-uniform loops of bkt_step and trie_walk)."""
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.setenv("COP_TBL8", "plain")
    ctx = gpu_ctx_factory(stages=S | F | L, flags=MODES[mode][0])
    load(ctx, "stride_edges", "crafted")
    assert ctx.route_form() == mode
    pk, n, ro, fo = batch("stride_edges", "crafted", S | F | L)
    reach = ~np.isin(ro["verdict"], (cg.DROP_PARSE, cg.DROP_NO_PORT))
    assert 0.90 <= reach.mean() < 1.0, reach.mean()
    rg, fg, _ = gpu_run(ctx, pk, n, batches=1)
    assert_parity(rg, fg, ro, fo)


def run_step_path(ctx, kname, n, pkts, ro, fo, offsets=None):
    """One ring slot through the poll-mode kernel, twice; records and
    segment lists against the oracle's."""
    dp = ctx.alloc(pkts.nbytes + (offsets.nbytes if offsets is not None else 0))
    dp.upload(pkts)
    dr = ctx.alloc(n * 8)
    df = ctx.alloc(n * 4)
    dc = ctx.alloc(nseg(n) * 4 + 16)
    dr.fill(0xEE)
    if offsets is not None:
        dp.upload(offsets, pkts.nbytes)
        ring = cg.make_ring(dp, 1, n, dr, dp.nbytes, offsets=dp.addr + pkts.nbytes,
                            offsets_slot_words=dp.nbytes // 4, fwd_idx=df, fwd_count=dc)
    else:
        ring = cg.make_ring(dp, 1, n, dr, n * 64, stride=64, fwd_idx=df, fwd_count=dc)
    with ctx.pmd_start(ring) as m:
        assert m.info()["kernel_name"] == kname, m.info()
        m.run(2)
    res = dr.download(cg.RESULT_DT, n)
    got = seg_to_dense(df.download(np.uint32, n), dc.download(np.uint32, nseg(n)), n)
    assert_parity(res, got, ro, fo)


STEP_FORMS = {"dir-plain": (0, "plain", 2), "dir-packed": (0, "packed", 2), "bkt": (cg.CFG_LPM_BKT, "plain", 4)}


@pytest.mark.parametrize("route", LARGE)
@pytest.mark.parametrize("form", list(STEP_FORMS))
def test_step_path_boundaries_slots(gpu_ctx_factory, monkeypatch, route, form):
    """The poll-mode step path (segmented lists, cop_tile.h tile_steps_v):
    the route's second round split across steps, tbl8_issue / tbl8_finish
    over plain and packed groups and bkt_pairs_issue / bkt_pairs_finish, the
    firewall in LDS; 64-byte slots, whole tiles."""
    flags, tbl8, lpm = STEP_FORMS[form]
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.setenv("COP_TBL8", tbl8)
    ctx = gpu_ctx_factory(stages=F | L, flags=flags | cg.CFG_SEG_LISTS)
    load(ctx, route, "crafted")
    pk, n, ro, fo = batch(route, "crafted", F | L, 1024)
    assert n % 1024 == 0
    run_step_path(ctx, f"cop_pmd<1, {lpm}, 2, 4, false>", n, pk, ro, fo)


@functools.lru_cache(maxsize=None)
def imix_batch(route, fw):
    p = probe_set(route, fw, 1024)
    slab, offs = cg.gen_imix(0x5EED0E03, len(p), None, None, opts=cg.trace_opts(**NO_PCT))
    le.write_headers(slab, offs, p, p[::-1])
    ro, fo, _ = orc.process(slab, len(p), offsets=offs, stages=F | L, fw=tables(fw, True)[1],
                            route=tables(route, False)[1])
    return slab, offs, len(p), ro, fo


@pytest.mark.parametrize("route,form", [("stride_edges", "dir-plain"), ("bkt_widths", "bkt")])
def test_step_path_boundaries_imix(gpu_ctx_factory, monkeypatch, route, form):
    """The same headers in an IMIX slab at its offsets: the step path's
    other layout."""
    flags, tbl8, lpm = STEP_FORMS[form]
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.setenv("COP_TBL8", tbl8)
    ctx = gpu_ctx_factory(stages=F | L, flags=flags | cg.CFG_SEG_LISTS)
    load(ctx, route, "crafted")
    slab, offs, n, ro, fo = imix_batch(route, "crafted")
    assert (ro["verdict"] != cg.DROP_NOT_IPV4).all()      # every probe reaches both lookups
    run_step_path(ctx, f"cop_pmd<1, {lpm}, 1, 4, false>", n, slab, ro, fo, offsets=offs)


def test_step_path_boundaries_route_in_lds(gpu_ctx_factory, monkeypatch):
    """Both tables in LDS on the poll-mode kernel (the probes repeated to
    4096 packets, the smallest batch that gets its 1024-packet tiles)."""
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.delenv("COP_TBL8", raising=False)
    ctx = gpu_ctx_factory(stages=F | L, flags=cg.CFG_SEG_LISTS)
    load(ctx, "crafted", "crafted")
    assert ctx.route_form() == "lds"
    pk, n, ro, fo = batch("crafted", "crafted", F | L, 4096)
    assert n == 4096
    run_step_path(ctx, "cop_pmd<1, 1, 2, 4, false>", n, pk, ro, fo)


def test_headline_engine_records(gpu_ctx_factory, monkeypatch):
    """The engine behind bench.py's line with its own declaration: stages
    S | F, the 1000-rule firewall in LDS, segmented lists, the poll-mode
    kernel started with PMD_STATIC_SLOTS over a 24-slot ring of
    65,536-packet batches, 20 batches posted at once. Slot 0 holds the
    firewall's boundary probes as sources (cycled), the others generator
    traffic; the records and segment lists of all 20 slots against the
    oracle (Weak 6: this instantiation had no record check)."""
    monkeypatch.delenv("COP_PPT", raising=False)
    rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    fwt = cg.LpmTable(rules, 1024, 24, True)
    ofw = orc.OracleLpm(1024, 24)
    ofw.setup(rules["ip"], rules["depth"], rules["next_hop"])
    B, P, N = 65536, 24, 20
    probes = le.boundary_probes(fwt)
    src = le.pad_to(probes, B)[:B]
    assert len(probes) <= B
    pk = np.concatenate([le.probe_frames(src), cg.gen_trace(0x5EED0E04, (P - 1) * B, rules, None)])
    ctx = gpu_ctx_factory(stages=S | F, max_batch=B, max_batches=32, flags=cg.CFG_SEG_LISTS)
    ctx.set_fw_table(fwt)
    dp = ctx.alloc(P * B * 64)
    dp.upload(pk)
    dr = ctx.alloc(P * B * 8)
    df = ctx.alloc(P * B * 4)
    dc = ctx.alloc(P * nseg(B) * 4 + 16)
    dr.fill(0xAB)
    ring = cg.make_ring(dp, P, B, dr, B * 64, stride=64, fwd_idx=df, fwd_count=dc)
    ctx.counters(reset=True)
    with ctx.pmd_start(ring, cg.PMD_STATIC_SLOTS) as m:
        info = m.info()
        assert info["kernel_name"] == "cop_pmd<1, 0, 2, 4, false>", info
        m.post(N)
        m.wait()
        info = m.info()
        assert info["slot_loads"] == 0 and info["completed"] == N, info
    res = dr.download(cg.RESULT_DT, P * B)
    fwd = df.download(np.uint32, P * B)
    cnt = dc.download(np.uint32, P * nseg(B))
    ns = nseg(B)
    for s in range(N):
        ro, fo, _ = orc.process(pk[s * B * 64:(s + 1) * B * 64], B, stages=S | F, fw=ofw)
        if s == 0:
            assert (ro["flags"] & 2).mean() > 0.3 and 0.05 < (ro["verdict"] == cg.DROP_FW).mean() < 0.95
        got = seg_to_dense(fwd[s * B:(s + 1) * B], cnt[s * ns:(s + 1) * ns], B)
        assert_parity(res[s * B:(s + 1) * B], got, ro, fo)
    assert (res[N * B:].view(np.uint8) == 0xAB).all()      # the slots never posted stay untouched
    assert ctx.counters()["rx"] == N * B
