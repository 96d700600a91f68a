"""GPU: live LPM rule updates (COP_CFG_LIVE_TABLES, cop_update_*).

The patch kernel alone against its numpy mirror; then whole updates: batches
submitted before an update must see the old rule set in every packet, batches
submitted after it the new one, with no sync in between, in the DIR-24-8 form,
in the LDS form, across the LDS limit, under the poll-mode kernel, through
the whole-table fallbacks and from an edited rules file. The expected records
are always the oracle's over a table built from the surviving rules
(live_tables.Model), the update script is live_tables.script().
"""
import numpy as np
import pytest

import copgpu as cg
import lpm_edges as le
import oracle as orc
from helpers import assert_parity
from live_tables import PATCH_SPAN, Model, ids_to_keys, script, script_tail, touched_addresses
from test_gpu_seg import nseg, seg_to_dense

pytestmark = pytest.mark.gpu

S, F, L = cg.STAGE_PARSE, cg.STAGE_FW, cg.STAGE_LPM
LIVE = cg.CFG_LIVE_TABLES
EBUSY = -16


class Job:
    """One batch with its own device buffers, allocated and uploaded before
    anything is submitted, so that nothing between two submits waits."""

    def __init__(self, ctx, pk, n):
        self.ctx, self.n = ctx, n
        self.dp = ctx.alloc(pk.nbytes)
        self.dp.upload(pk)
        self.dr, self.df, self.dc = ctx.alloc(n * 8), ctx.alloc(n * 4), ctx.alloc(16)
        self.dr.fill(0xAB)
        self.dc.fill(0xFF)

    def submit(self):
        self.ctx.submit([cg.make_batch(self.dp, self.n, self.dr, fwd_idx=self.df, fwd_count=self.dc)])

    def result(self):
        cnt = int(self.dc.download(np.uint32, 1)[0])
        assert cnt <= self.n
        return self.dr.download(cg.RESULT_DT, self.n), self.df.download(np.uint32, cnt)


def script_rules(groups) -> np.ndarray:
    ops = [op for g in groups for op in g if op[0] == "add"]
    return cg.prefixes([op[1] for op in ops], [op[2] for op in ops], [op[3] for op in ops])


def probe_batch(rule_sets, multiple=1024):
    """Frames over the boundary probes of all rule_sets and every address the
    script touches: sources ascending, destinations descending."""
    parts = [le.boundary_probes(r) for r in rule_sets] + [touched_addresses()]
    p = le.pad_to(le.subsample(np.unique(np.concatenate(parts))), multiple)
    return le.probe_frames(p), len(p)


def expect(pk, n, stages, mfw, mrt, hits=False):
    ofw, ort = mfw.oracle() if mfw else None, mrt.oracle() if mrt else None
    h = np.zeros(max(ofw.n_rules, 1), np.uint64) if hits else None
    ro, fo, co = orc.process(pk, n, stages=stages, fw=ofw, route=ort, rule_hits=h)
    return ro, fo, co, ofw, h


# ---- f. the kernel alone -----------------------------------------------------
def kernel_records(caps, seed=0x9A7C4) -> np.ndarray:
    """3,000 disjoint fill records in random order: in tbl24 (caps[0]
    entries) runs of 1, 2, 3, 4, 5, 122, PATCH_SPAN - 1 .. PATCH_SPAN + 1 and
    2046 .. 2049 entries at each start alignment 0..3, then random runs of 1
    to 5,000 entries; in tbl8 (caps[1]) a few long runs, then thousands of
    runs of 1 to 7 entries, as a burst of host-route changes makes them."""
    rng = np.random.default_rng(seed)
    crafted = [c for a in range(4) for c in (1, 2, 3, 4, 5, 122, PATCH_SPAN - 1, PATCH_SPAN, PATCH_SPAN + 1, 2046,
                                                 2047, 2048, 2049)]
    recs = []
    for tb, cap, n_runs in ((0, caps[0], 200), (1, caps[1] // 2, 12)):
        pos, k = 0, 0
        counts = crafted[:] if tb == 0 else [1, 1, 1, 122, 255, 256]
        while len(counts) < n_runs:
            counts.append(int(rng.integers(1, 5001)))
        for c in counts:
            first = pos + int(rng.integers(0, 40))
            if tb == 0 and k < len(crafted):
                first = (first + 3) // 4 * 4 + k // 13           # the crafted counts at alignments 0..3
            if first + c > cap:
                break
            recs.append((tb, first, c, int(rng.integers(0, 1 << 32))))
            pos, k = first + c, k + 1
    pos = caps[1] // 2 + 5                                       # the short runs: tbl8's second half
    for _ in range(3000 - len(recs)):
        first = pos + int(rng.integers(0, 4))
        c = int(rng.integers(1, 8))
        recs.append((1, first, c, int(rng.integers(0, 1 << 32))))
        pos = first + c
    assert pos <= caps[1]
    recs = np.array(recs, dtype=cg.PATCH_REC_DT)
    return recs[rng.permutation(len(recs))]


def test_patch_kernel_against_the_numpy_mirror(gpu_ctx_factory):
    """The kernel through cop_debug_patch on buffers of 2^20 and 2^16 entries
    filled with 0xAB: every word, written or not, equals the host mirror's."""
    ctx = gpu_ctx_factory(stages=S)
    caps = (1 << 20, 1 << 16)
    recs = kernel_records(caps)
    assert len(recs) == 3000 and {int(f) % 4 for f in recs["first"]} == {0, 1, 2, 3}
    assert (recs["count"] == 1).sum() > 200 and recs["count"].max() > 4000
    d24, d8 = ctx.alloc(caps[0] * 4), ctx.alloc(caps[1] * 4)
    d24.fill(0xAB)
    d8.fill(0xAB)
    h24, h8 = np.full(caps[0], 0xABABABAB, np.uint32), np.full(caps[1], 0xABABABAB, np.uint32)
    cg.patch_apply_host(h24, h8, recs)
    sent = ctx.debug_patch(d24, d8, recs)
    assert sent > len(recs)                                   # long runs were cut
    assert np.array_equal(d24.download(np.uint32, caps[0]), h24)
    assert np.array_equal(d8.download(np.uint32, caps[1]), h8)
    assert (h24 == 0xABABABAB).sum() > 1000 and (h8 == 0xABABABAB).sum() > 1000
    # a record that leaves its table is refused whole
    bad = np.array([(0, caps[0] - 2, 3, 7)], dtype=cg.PATCH_REC_DT)
    with pytest.raises(cg.CopError):
        ctx.debug_patch(d24, d8, bad)
    assert np.array_equal(d24.download(np.uint32, caps[0]), h24)


# ---- g. one-shot ordering, DIR form ------------------------------------------
def test_oneshot_ordering_dir_form(gpu_ctx_factory, monkeypatch):
    """Batch A, the script as one update per step group for both stages with
    no sync, batch B on the other lane, delete_all + ten rules, batch C, one
    sync: A is served by the old tables, B by the script's, C by the last."""
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.setenv("COP_TBL8", "packed")                 # ignored on a live context
    rules = np.concatenate([le.filler(), le.stride_edges_crafted()])
    fwr = le.fw_rules(rules)
    tfw, trt = le.table(fwr), le.table(rules)
    mfw, mrt = Model(tfw, *le.RT_CFG[:2], rules=fwr), Model(trt, *le.RT_CFG[:2], rules=rules)
    ctx = gpu_ctx_factory(stages=F | L, flags=LIVE | cg.CFG_RULE_COUNTERS, n_streams=2)
    ctx.set_fw_table(tfw)
    ctx.set_route_lpm(trt)
    assert ctx.route_form() == "dir"
    pk, n = probe_batch([rules, script_rules(script() + script_tail())])
    assert n % 1024 == 0
    ja, jb, jc = Job(ctx, pk, n), Job(ctx, pk, n), Job(ctx, pk, n)
    ea = expect(pk, n, F | L, mfw, mrt)
    ctx.counters(reset=True)
    ctx.rule_counters(reset=True)

    reps = []
    ja.submit()
    for group in script():
        mfw.run(group)
        mrt.run(group)
        reps += [ctx.update_fw_table(tfw), ctx.update_route_lpm(trt)]
    jb.submit()
    assert ctx.route_form() == "dir"
    eb = expect(pk, n, F | L, mfw, mrt)
    for group in script_tail():
        mfw.run(group)
        mrt.run(group)
        reps += [ctx.update_fw_table(tfw), ctx.update_route_lpm(trt)]
    assert ctx.route_form() == "lds"                         # ten rules: the table changed form at the update
    jc.submit()
    ctx.sync()

    ec = expect(pk, n, F | L, mfw, mrt, hits=True)
    for r in reps:
        assert r["full"] == 0 and r["n_changes"] > 0, r
        assert r["h2d_bytes"] <= 16 * r["n_records"] + 4096, r
    assert sum(r["groups_taken"] for r in reps) >= 6 and sum(r["groups_released"] for r in reps) >= 6
    assert max(r["tbl24_entries"] for r in reps) >= 1 << 23        # the /1
    # an update that did nothing would fail: the oracles alone say the batches differ
    assert ((ea[0]["verdict"] != eb[0]["verdict"]) | (ea[0]["route_nh"] != eb[0]["route_nh"])).sum() >= 100
    assert ((eb[0]["verdict"] != ec[0]["verdict"]) | (eb[0]["route_nh"] != ec[0]["route_nh"])).sum() >= 100
    for job, e in ((ja, ea), (jb, eb), (jc, ec)):
        rg, fg = job.result()
        assert_parity(rg, fg, e[0], e[1])
    got = ctx.counters()
    for k in got:
        assert got[k] == ea[2][k] + eb[2][k] + ec[2][k], k
    # per-rule counters by (prefix, depth): delete_all zeroed every word in the
    # patch's order, so they hold batch C's hits alone, under the new ids
    ctr = ctx.rule_counters()
    assert len(ctr) == le.RT_CFG[0]
    r, ids = tfw.rules_ids()
    assert len(r) == 10
    oip, od, _ = ec[3].rules_by_id()
    want = dict(zip(ids_to_keys(np.arange(len(oip)), oip, od).tolist(), ec[4][:len(oip)].tolist()))
    for key, i in zip(ids_to_keys(ids, r["ip"], r["depth"], ids).tolist(), ids.tolist()):
        assert int(ctr[i]) == want[key], (hex(key), i)
    assert int(ctr.sum()) == int(ec[4].sum()) > 0


def test_rule_counters_follow_their_ids(gpu_ctx_factory):
    """fw1k with per-rule counters: rules 3, 7 and 11 are deleted, two new
    rules take ids 3 and 7, one action flips. Kept rules count both batches,
    the new rules in the reused ids the second batch alone, the freed id 11
    reads zero."""
    rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    t = cg.LpmTable(rules, 1024, 24, True)
    m = Model(t, 1024, 24, rules=rules)
    ctx = gpu_ctx_factory(stages=F, flags=LIVE | cg.CFG_RULE_COUNTERS, n_streams=2)
    ctx.set_fw_table(t)
    r0, _ = t.rules_ids()
    new = cg.prefixes([0xC6338000, 0xC6336400], [25, 24], [1, 1])
    pk, n = probe_batch([r0, new])
    ja, jb = Job(ctx, pk, n), Job(ctx, pk, n)
    ea = expect(pk, n, F, m, None, hits=True)
    ja.submit()
    for k in (3, 7, 11):
        m.delete(int(r0["ip"][k]), int(r0["depth"][k]))
    for p in new:
        m.add(int(p["ip"]), int(p["depth"]), int(p["next_hop"]))
    m.add(int(r0["ip"][20]), int(r0["depth"][20]), 0 if r0["next_hop"][20] else 1)
    rep = ctx.update_fw_table(t)
    jb.submit()
    ctx.sync()
    eb = expect(pk, n, F, m, None, hits=True)
    assert rep["full"] == 0 and rep["n_changes"] == 6
    for job, e in ((ja, ea), (jb, eb)):
        rg, fg = job.result()
        assert_parity(rg, fg, e[0], e[1])
    r1, ids1 = t.rules_ids()
    assert {3, 7} <= set(ids1.tolist()) and 11 not in ids1.tolist()
    ctr = ctx.rule_counters()
    assert len(ctr) == 1024 and ctr[11] == 0
    ka = dict(zip(ids_to_keys(np.arange(len(r0)), r0["ip"], r0["depth"]).tolist(), ea[4].tolist()))
    oip, od, _ = eb[3].rules_by_id()
    kb = dict(zip(ids_to_keys(np.arange(len(oip)), oip, od).tolist(), eb[4].tolist()))
    fresh = set(ids_to_keys(np.arange(2), new["ip"], new["depth"]).tolist())
    assert sum(kb[k] for k in fresh) > 0 and sum(ea[4][[3, 7, 11]]) > 0
    for key, i in zip(ids_to_keys(ids1, r1["ip"], r1["depth"], ids1).tolist(), ids1.tolist()):
        assert int(ctr[i]) == kb[key] + (0 if key in fresh else ka[key]), (hex(key), i)


# ---- h. LDS form ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["crafted", "fw1k"])
def test_oneshot_ordering_lds_form(gpu_ctx_factory, monkeypatch, name):
    """The same script on tables that stay in LDS: the interval image is
    rebuilt and copied in stream order with every update."""
    monkeypatch.delenv("COP_PPT", raising=False)
    rules, cfg = le.small_tables()[name]
    fwr = le.fw_rules(rules) if name == "crafted" else rules
    tfw, trt = le.table(fwr, cfg), le.table(rules, cfg)
    lim = (max(cfg[0], len(rules)), cfg[1])
    mfw, mrt = Model(tfw, *lim, rules=fwr), Model(trt, *lim, rules=rules)
    ctx = gpu_ctx_factory(stages=F | L, flags=LIVE, n_streams=2)
    ctx.set_fw_table(tfw)
    ctx.set_route_lpm(trt)
    assert ctx.route_form() == "lds"
    pk, n = probe_batch([rules, script_rules(script() + script_tail())])
    ja, jb, jc = Job(ctx, pk, n), Job(ctx, pk, n), Job(ctx, pk, n)
    ea = expect(pk, n, F | L, mfw, mrt)
    reps = []
    ja.submit()
    for group in script():
        mfw.run(group)
        mrt.run(group)
        reps += [ctx.update_fw_table(tfw), ctx.update_route_lpm(trt)]
    jb.submit()
    eb = expect(pk, n, F | L, mfw, mrt)
    for group in script_tail():
        mfw.run(group)
        mrt.run(group)
        reps += [ctx.update_fw_table(tfw), ctx.update_route_lpm(trt)]
    jc.submit()
    ctx.sync()
    ec = expect(pk, n, F | L, mfw, mrt)
    assert all(r["full"] == 0 for r in reps), reps
    assert ctx.route_form() == "lds"
    assert ((ea[0]["verdict"] != eb[0]["verdict"]) | (ea[0]["route_nh"] != eb[0]["route_nh"])).sum() >= 100
    for job, e in ((ja, ea), (jb, eb), (jc, ec)):
        rg, fg = job.result()
        assert_parity(rg, fg, e[0], e[1])


def test_update_across_the_lds_limit(gpu_ctx_factory, monkeypatch):
    """8192 intervals sit in LDS; one more host route takes the table to the
    DIR-24-8 form at the update, deleting it brings the LDS form back."""
    monkeypatch.delenv("COP_PPT", raising=False)
    rules = le.lds_limit(4096)
    trt = le.table(rules)
    mrt = Model(trt, *le.RT_CFG[:2], rules=rules)
    ctx = gpu_ctx_factory(stages=F | L, flags=LIVE, n_streams=2)
    ctx.set_route_lpm(trt)
    assert ctx.route_form() == "lds" and trt.report.n_intervals == le.IVT_MAX
    host = cg.prefixes([0x7F000001], [32], [77])
    pk, n = probe_batch([rules, host])
    jobs = [Job(ctx, pk, n) for _ in range(3)]
    exp = [expect(pk, n, F | L, None, mrt)]
    jobs[0].submit()
    mrt.add(0x7F000001, 32, 77)
    assert trt.report.n_intervals == le.IVT_MAX + 2
    r1 = ctx.update_route_lpm(trt)
    assert ctx.route_form() == "dir"
    jobs[1].submit()
    exp.append(expect(pk, n, F | L, None, mrt))
    mrt.delete(0x7F000001, 32)
    r2 = ctx.update_route_lpm(trt)
    assert ctx.route_form() == "lds"
    jobs[2].submit()
    ctx.sync()
    exp.append(exp[0])
    assert r1["full"] == 0 and r2["full"] == 0
    assert (exp[0][0]["route_nh"] != exp[1][0]["route_nh"]).sum() >= 1
    for job, e in zip(jobs, exp):
        rg, fg = job.result()
        assert_parity(rg, fg, e[0], e[1])


# ---- i. under the poll-mode kernel -------------------------------------------
def test_update_under_the_poll_mode_kernel(gpu_ctx_factory, monkeypatch):
    """fw1k in LDS, a 2-slot ring of 4096-packet batches: post, wait, update
    eight rules (four actions flipped, two rules deleted, two added), post,
    wait: slot 0 was served by the old table, slot 1 by the new one, by the
    same kernel. Then an update that changes the launch geometry
    (delete_all: another LDS image size) returns -EBUSY and leaves the device
    on the table it had."""
    monkeypatch.delenv("COP_PPT", raising=False)
    rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    t = cg.LpmTable(rules, 1024, 24, True)
    m = Model(t, 1024, 24, rules=rules)
    r0 = t.rules()
    new = cg.prefixes([0xC6336400, 0xC6336480], [24, 25], [1, 0])
    changed = np.concatenate([r0[[5, 6, 8, 9, 30, 31]], new])
    B = 4096
    rest = le.subsample(le.boundary_probes(r0), B - 6 * len(changed) - 4)
    p = le.pad_to(np.unique(np.concatenate([le.boundary_probes(changed), rest])), B)[:B]
    pk = le.probe_frames(p)
    ctx = gpu_ctx_factory(stages=F, flags=cg.CFG_SEG_LISTS | LIVE, max_batch=B)
    ctx.set_fw_table(t)
    dp = ctx.alloc(2 * B * 64)
    dp.upload(np.concatenate([pk, pk]))
    dr, df, dc = ctx.alloc(2 * B * 8), ctx.alloc(2 * B * 4), ctx.alloc(2 * nseg(B) * 4 + 16)
    dr.fill(0xAB)
    ring = cg.make_ring(dp, 2, B, dr, B * 64, stride=64, fwd_idx=df, fwd_count=dc)

    def slot(s):
        res = dr.download(cg.RESULT_DT, 2 * B)[s * B:(s + 1) * B]
        fwd = df.download(np.uint32, 2 * B)[s * B:(s + 1) * B]
        cnt = dc.download(np.uint32, 2 * nseg(B))[s * nseg(B):(s + 1) * nseg(B)]
        return res, seg_to_dense(fwd, cnt, B)

    e0 = expect(pk, B, F, m, None)
    with ctx.pmd_start(ring) as pm:
        name = pm.info()["kernel_name"]
        pm.post(1)
        pm.wait()
        for k in (5, 6, 8, 9):
            m.add(int(r0["ip"][k]), int(r0["depth"][k]), 0 if r0["next_hop"][k] else 1)
        for k in (30, 31):
            m.delete(int(r0["ip"][k]), int(r0["depth"][k]))
        for q in new:
            m.add(int(q["ip"]), int(q["depth"]), int(q["next_hop"]))
        rep = ctx.update_fw_table(t)
        pm.post(1)
        pm.wait()
        info = pm.info()
    e1 = expect(pk, B, F, m, None)
    assert rep["full"] == 0 and rep["n_changes"] == 8, rep
    assert info["kernel_name"] == name and info["completed"] == 2, info
    assert (e0[0]["verdict"] != e1[0]["verdict"]).sum() >= 8
    assert_parity(*slot(0), e0[0], e0[1])
    assert_parity(*slot(1), e1[0], e1[1])
    # a geometry change is refused, and the device keeps the table it had
    dr.fill(0xAB)
    with ctx.pmd_start(ring) as pm:
        assert pm.info()["kernel_name"] == name
        pm.post(1)
        pm.wait()
        m.delete_all()
        with pytest.raises(cg.CopError) as err:
            ctx.update_fw_table(t)
        assert err.value.code == EBUSY
        pm.post(1)
        pm.wait()
        info = pm.info()
    assert info["kernel_name"] == name and info["completed"] == 2, info
    assert_parity(*slot(0), e1[0], e1[1])
    assert_parity(*slot(1), e1[0], e1[1])
    # with the kernel stopped the same update goes through
    rep = ctx.update_fw_table(t)
    assert rep["full"] == 0
    ja = Job(ctx, pk, B)
    ctx2 = expect(pk, B, F, m, None)
    ctx.submit([cg.make_batch(ja.dp, B, ja.dr)])
    ctx.sync()
    res = ja.dr.download(cg.RESULT_DT, B)
    assert np.array_equal(res["verdict"], ctx2[0]["verdict"]) and (res["verdict"] == cg.FORWARD).all()


def test_rule_counters_refuse_table_changes_under_the_poll_mode_kernel(gpu_ctx_factory, monkeypatch):
    """fw1k in LDS with per-rule counters, a 2-slot ring of 4096-packet
    batches. With the kernel serving, an update (one rule added) and a
    replacement (every action flipped) are both refused with -EBUSY before the
    kernel is paused, and both slots are served by the table as first set.
    With the kernel stopped the same update and the same replacement go down
    the device path and the stage audits clean against each table."""
    monkeypatch.delenv("COP_PPT", raising=False)
    rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    flipped = rules.copy()
    flipped["next_hop"] = np.where(rules["next_hop"] != 0, 0, 1)
    a, b = cg.LpmTable(rules, 1024, 24, True), cg.LpmTable(flipped, 1024, 24, True)
    m = Model(a, 1024, 24, rules=rules)
    new = cg.prefixes([0xC6336400], [24], [1])
    B = 4096
    rest = le.subsample(le.boundary_probes(a.rules()), B - 6 * len(new) - 4)
    pk = le.probe_frames(le.pad_to(np.unique(np.concatenate([le.boundary_probes(new), rest])), B)[:B])
    ctx = gpu_ctx_factory(stages=F, flags=LIVE | cg.CFG_RULE_COUNTERS | cg.CFG_SEG_LISTS, max_batch=B)
    ctx.set_fw_table(a)
    dp = ctx.alloc(2 * B * 64)
    dp.upload(np.concatenate([pk, pk]))
    dr, df, dc = ctx.alloc(2 * B * 8), ctx.alloc(2 * B * 4), ctx.alloc(2 * nseg(B) * 4 + 16)
    dr.fill(0xAB)
    ring = cg.make_ring(dp, 2, B, dr, B * 64, stride=64, fwd_idx=df, fwd_count=dc)

    def slot(s):
        res = dr.download(cg.RESULT_DT, 2 * B)[s * B:(s + 1) * B]
        fwd = df.download(np.uint32, 2 * B)[s * B:(s + 1) * B]
        cnt = dc.download(np.uint32, 2 * nseg(B))[s * nseg(B):(s + 1) * nseg(B)]
        return res, seg_to_dense(fwd, cnt, B)

    def audit(tab):
        rep, bad = ctx.lookup_audit(F, tab, bad_cap=8)
        assert rep["n_mismatch"] == 0 and rep["stale"] == 0 and rep["n_probes"] > 0, (rep, bad)

    e0 = expect(pk, B, F, m, None)
    with ctx.pmd_start(ring) as pm:
        pm.post(1)
        pm.wait()
        m.add(int(new["ip"][0]), int(new["depth"][0]), int(new["next_hop"][0]))
        before = pm.info()["launches"]
        for change, tab in ((ctx.update_fw_table, a), (ctx.replace_fw_table, b)):
            with pytest.raises(cg.CopError) as err:
                change(tab)
            assert err.value.code == EBUSY and "per-rule counters" in str(err.value), str(err.value)
        assert pm.info()["launches"] == before                   # nothing was paused
        pm.post(1)
        pm.wait()
        assert pm.info()["completed"] == 2
    eb = expect(pk, B, F, Model(b, 1024, 24, rules=flipped), None)
    assert (e0[0]["verdict"] != eb[0]["verdict"]).sum() >= 100   # a replacement that got through would show
    assert_parity(*slot(0), e0[0], e0[1])
    assert_parity(*slot(1), e0[0], e0[1])
    # with the kernel stopped both changes take the device path
    assert ctx.update_fw_table(a)["full"] == 0
    audit(a)
    assert ctx.replace_fw_table(b)["full"] == 0
    audit(b)


# ---- j. fallbacks ---------------------------------------------------------------
@pytest.mark.parametrize("case", ["not_live", "route_bkt", "foreign_table"])
def test_update_falls_back_to_the_whole_upload(gpu_ctx_factory, monkeypatch, case):
    monkeypatch.delenv("COP_PPT", raising=False)
    rules = np.concatenate([le.filler(), le.stride_edges_crafted()]) if case == "route_bkt" else le.stride_edges_crafted()
    trt = le.table(rules)
    mrt = Model(trt, *le.RT_CFG[:2], rules=rules)
    flags = {"not_live": 0, "route_bkt": LIVE | cg.CFG_LPM_BKT, "foreign_table": LIVE}[case]
    ctx = gpu_ctx_factory(stages=F | L, flags=flags)
    ctx.set_route_lpm(trt)
    assert ctx.route_form() == ("bkt" if case == "route_bkt" else "lds")
    group = script()[0] + script()[7]
    if case == "foreign_table":
        trt = le.table(rules)                                  # another table object with the same rules
        mrt = Model(trt, *le.RT_CFG[:2], rules=rules)
    mrt.run(group)
    pk, n = probe_batch([rules, script_rules([group])])
    rep = ctx.update_route_lpm(trt)
    assert rep["full"] == 1 and rep["n_records"] == 0 and rep["h2d_bytes"] >= 4 << 24, rep
    job = Job(ctx, pk, n)
    job.submit()
    ctx.sync()
    e = expect(pk, n, F | L, None, mrt)
    assert_parity(*job.result(), e[0], e[1])
    if case == "foreign_table":
        # the context holds the new table now: its next change is a patch
        mrt.run(script()[1])
        assert ctx.update_route_lpm(trt)["full"] == 0


# ---- k. the rules file ---------------------------------------------------------
def test_update_fw_rules_file(gpu_ctx_factory, tmp_path):
    rules = cg.gen_rules(0x5EED1002, 200, cg.GEN_FW, 8)
    path = str(tmp_path / "rules.json")
    cg.rules_write_json(path, rules)
    t = cg.LpmTable(cg.rules_load_json(path), 1024, 24, True)
    ctx = gpu_ctx_factory(stages=F, flags=LIVE)
    ctx.set_fw_table(t)
    held = t.rules()
    edited = held[[i for i in range(len(held)) if i not in (2, 50, 120)]].copy()      # remove 3
    for k in (10, 60):                                                                # change 2 actions
        edited["next_hop"][k] = 0 if edited["next_hop"][k] else 1
    edited = np.concatenate([edited, cg.prefixes([0xC6336400, 0xC6336480, 0xC0A80000], [24, 26, 16], [1, 0, 1])])
    cg.rules_write_json(path, edited)
    g = t.generation
    rep = ctx.update_fw_rules_file(t, path)
    assert rep["full"] == 0 and rep["n_changes"] == 8 == t.generation - g, rep
    o = orc.OracleLpm(1024, 24)
    for ip, depth, action in orc.load_rules_json(path):
        if o.add(ip, depth, action) != 0:
            break
    pk, n = probe_batch([held, edited])
    ro, fo, _ = orc.process(pk, n, stages=F, fw=o)
    job = Job(ctx, pk, n)
    job.submit()
    ctx.sync()
    assert_parity(*job.result(), ro, fo)
    oip, od, onh = o.rules()
    mine = t.rules()
    order = np.lexsort((mine["depth"], mine["ip"]))
    assert np.array_equal(mine["ip"][order], oip) and np.array_equal(mine["depth"][order], od)
    assert np.array_equal(mine["next_hop"][order], onh)
