"""GPU: a stage's whole table replaced in stream order (cop_replace_*), the
DIR-24-8 image painted on the device from the table's intervals.

The paint kernel alone against its host mirror; then whole replacements:
batches submitted before one must see the old table in every packet, batches
submitted after it the new one, with no sync in between, in the DIR-24-8
form, in the LDS form and across the LDS limit, with the table's journal cut,
under the poll-mode kernel, through the whole-upload fallbacks, and across a
tbl8 buffer the new table outgrows. The expected records are always the
oracle's over the rule set the stage should hold.
"""
import numpy as np
import pytest

import copgpu as cg
import lpm_edges as le
import oracle as orc
import paint_tables as pt
from helpers import assert_parity
from live_tables import ids_to_keys
from test_gpu_live_tables import Job
from test_gpu_seg import nseg, seg_to_dense

pytestmark = pytest.mark.gpu

S, F, L = cg.STAGE_PARSE, cg.STAGE_FW, cg.STAGE_LPM
LIVE = cg.CFG_LIVE_TABLES
EBUSY, EINVAL = -16, -22
FW1K_CFG = (1024, 24, True)


class Tab:
    """A rule set as a table object and as the oracle's table."""

    def __init__(self, rules, cfg=le.RT_CFG):
        self.rules, self.cfg = rules, cfg
        self.t = le.table(rules, cfg)
        self.o = orc.OracleLpm(max(cfg[0], len(rules), 1), cfg[1])
        if len(rules):
            self.o.setup(rules["ip"], rules["depth"], rules["next_hop"], stop_at_error=cfg[2])


def probes(rule_sets, multiple=1024):
    p = np.unique(np.concatenate([le.boundary_probes(r) for r in rule_sets]))
    p = le.pad_to(le.subsample(p), multiple)
    return le.probe_frames(p), len(p)


def expect(pk, n, stages, fw=None, rt=None, hits=False):
    h = np.zeros(max(fw.o.n_rules, 1), np.uint64) if hits else None
    ro, fo, _ = orc.process(pk, n, stages=stages, fw=fw.o if fw else None, route=rt.o if rt else None, rule_hits=h)
    return ro, fo, h


def differ(a, b):
    return int(((a[0]["verdict"] != b[0]["verdict"]) | (a[0]["route_nh"] != b[0]["route_nh"])).sum())


def clean(ctx, stage, tab):
    rep, bad = ctx.lookup_audit(stage, tab.t, bad_cap=8)
    assert rep["n_mismatch"] == 0 and rep["stale"] == 0 and rep["n_probes"] > 0, (rep, bad)


# ---- 1. the kernel alone -----------------------------------------------------
@pytest.fixture(scope="module")
def paint_cases():
    """name -> (starts, entries, ext24, cap_groups, host tbl24, host tbl8): computed once."""
    out = {}
    for name, rules, form in (("crafted", pt.crafted(), le.FORM_NH), ("fw2000", pt.fw2000(), le.FORM_RULE),
                              ("routes20k", pt.routes20k(), le.FORM_NH)):
        s, e, x = cg.paint_plan(le.table(rules), form)
        cap = len(x) + 3
        out[name] = (s, e, x, cap) + cg.paint_host(s, e, x, cap)
    return out


@pytest.mark.parametrize("name", ["crafted", "fw2000", "routes20k"])
def test_paint_kernel_against_the_host_mirror(gpu_ctx_factory, paint_cases, name):
    """cop_debug_paint on a 64 MiB tbl24 and a tbl8 of cap_groups + 1 groups,
    both filled with 0xAB: every word equals the host paint, the group past
    cap_groups is untouched, and n_ext > cap_groups is refused whole."""
    s, e, x, cap, h24, h8 = paint_cases[name]
    assert len(x) > 0 and len(s) > 256
    ctx = gpu_ctx_factory(stages=S)
    d24, d8 = ctx.alloc(4 << 24), ctx.alloc((cap + 1) * 1024)
    d24.fill(0xAB)
    d8.fill(0xAB)
    with pytest.raises(cg.CopError) as err:
        ctx.debug_paint(s, e, x, d24, d8, len(x) - 1)
    assert err.value.code == EINVAL
    assert (d24.download(np.uint32, 1 << 24) == 0xABABABAB).all()
    assert (d8.download(np.uint32, (cap + 1) * 256) == 0xABABABAB).all()
    ctx.debug_paint(s, e, x, d24, d8, cap)
    g24, g8 = d24.download(np.uint32, 1 << 24), d8.download(np.uint32, (cap + 1) * 256)
    assert np.array_equal(g24, h24), np.nonzero(g24 != h24)[0][:8]
    assert np.array_equal(g8[:cap * 256], h8), np.nonzero(g8[:cap * 256] != h8)[0][:8]
    assert not g8[len(x) * 256:cap * 256].any()
    assert (g8[cap * 256:] == 0xABABABAB).all()


# ---- 2. one-shot ordering, DIR form ------------------------------------------
def test_oneshot_ordering_dir_form(gpu_ctx_factory, monkeypatch):
    """Job 1, both stages replaced by unrelated tables, job 2 on the other
    lane, one sync: job 1 is served by A in every packet, job 2 by B; the
    per-rule counters hold job 2's hits alone."""
    monkeypatch.delenv("COP_PPT", raising=False)
    ra = np.concatenate([le.filler(), le.stride_edges_crafted()])
    rb = np.concatenate([pt.routes20k()[:5000], pt.crafted()])
    afw, art, bfw, brt = Tab(le.fw_rules(ra)), Tab(ra), Tab(le.fw_rules(rb)), Tab(rb)
    ctx = gpu_ctx_factory(stages=F | L, n_streams=2,
                          flags=LIVE | cg.CFG_RULE_COUNTERS | cg.CFG_FW_FORCE_DIR24 | cg.CFG_LPM_FORCE_DIR24)
    ctx.set_fw_table(afw.t)
    ctx.set_route_lpm(art.t)
    assert ctx.lookup_form(F) == "dir" and ctx.lookup_form(L) == "dir"
    pk, n = probes([ra, rb])
    j1, j2 = Job(ctx, pk, n), Job(ctx, pk, n)
    e1, e2 = expect(pk, n, F | L, afw, art), expect(pk, n, F | L, bfw, brt, hits=True)
    assert differ(e1, e2) >= 100          # a replacement that did nothing would fail
    ctx.rule_counters(reset=True)

    j1.submit()
    reps = [ctx.replace_fw_table(bfw.t), ctx.replace_route_lpm(brt.t)]
    j2.submit()
    ctx.sync()

    for job, e in ((j1, e1), (j2, e2)):
        rg, fg = job.result()
        assert_parity(rg, fg, e[0], e[1])
    for r, b, form in zip(reps, (bfw, brt), (le.FORM_RULE, le.FORM_NH)):
        n_ext = pt.form_n_ext(b.t, form)
        assert r["full"] == 0 and r["n_changes"] == 0 and r["tbl24_entries"] == 1 << 24, r
        assert r["h2d_bytes"] < 1 << 20 and r["n_records"] == len(cg.paint_plan(b.t, form)[0]), r
        assert r["groups_taken"] == n_ext and r["tbl8_entries"] == n_ext * 256 and r["groups_released"] > 0, r
    # per-rule counters by (prefix, depth): job 1's hits were zeroed in the replacement's order
    ctr = ctx.rule_counters()
    r, ids = bfw.t.rules_ids()
    oip, od, _ = bfw.o.rules_by_id()
    want = dict(zip(ids_to_keys(np.arange(len(oip)), oip, od).tolist(), e2[2][:len(oip)].tolist()))
    for key, i in zip(ids_to_keys(ids, r["ip"], r["depth"], ids).tolist(), ids.tolist()):
        assert int(ctr[i]) == want[key], (hex(key), i)
    assert int(ctr.sum()) == int(e2[2].sum()) > 0
    clean(ctx, F, bfw)
    clean(ctx, L, brt)
    # the stage holds B with a fresh book: its next change is a patch
    assert bfw.t.add(0xC6336400, 26, 1) == 0
    rep = ctx.update_fw_table(bfw.t)
    assert rep["full"] == 0 and rep["n_records"] >= 1, rep
    clean(ctx, F, bfw)


# ---- 3. the LDS form and across the 8,192-interval limit -----------------------
def test_lds_form_and_across_the_limit(gpu_ctx_factory, monkeypatch):
    """Both stages in LDS take other LDS tables; the route stage then crosses
    the interval limit to the DIR-24-8 form and comes back."""
    monkeypatch.delenv("COP_PPT", raising=False)
    fw0, fw1 = Tab(le.fw_rules(le.stride_edges_crafted())), Tab(le.small_tables()["fw1k"][0], FW1K_CFG)
    rts = [Tab(le.lds_limit(4096)), Tab(le.small_tables()["halves"][0]), Tab(le.lds_limit(4097)),
           Tab(le.lds_limit(4096))]
    assert rts[0].t.report.n_intervals == le.IVT_MAX and rts[2].t.report.n_intervals == le.IVT_MAX + 2
    ctx = gpu_ctx_factory(stages=F | L, flags=LIVE, n_streams=2)
    ctx.set_fw_table(fw0.t)
    ctx.set_route_lpm(rts[0].t)
    assert ctx.lookup_form(F) == "lds" and ctx.lookup_form(L) == "lds"
    pk, n = probes([fw0.rules, fw1.rules] + [r.rules for r in rts[:3]])
    jobs = [Job(ctx, pk, n) for _ in range(4)]
    exp = [expect(pk, n, F | L, fw0, rts[0]), expect(pk, n, F | L, fw1, rts[1]), expect(pk, n, F | L, fw1, rts[2]),
           expect(pk, n, F | L, fw1, rts[3])]
    forms, reps = [], []
    jobs[0].submit()
    reps += [ctx.replace_fw_table(fw1.t), ctx.replace_route_lpm(rts[1].t)]
    forms.append((ctx.lookup_form(F), ctx.lookup_form(L)))
    jobs[1].submit()
    reps.append(ctx.replace_route_lpm(rts[2].t))
    forms.append((ctx.lookup_form(F), ctx.lookup_form(L)))
    jobs[2].submit()
    reps.append(ctx.replace_route_lpm(rts[3].t))
    forms.append((ctx.lookup_form(F), ctx.lookup_form(L)))
    jobs[3].submit()
    ctx.sync()
    assert forms == [("lds", "lds"), ("lds", "dir"), ("lds", "lds")], forms
    assert all(r["full"] == 0 and r["tbl24_entries"] == 1 << 24 for r in reps), reps
    assert min(differ(exp[i], exp[i + 1]) for i in range(3)) >= 1
    for job, e in zip(jobs, exp):
        rg, fg = job.result()
        assert_parity(rg, fg, e[0], e[1])
    clean(ctx, F, fw1)
    clean(ctx, L, rts[3])


# ---- 4. the same table object with its journal cut -----------------------------
def test_same_table_with_its_journal_cut(gpu_ctx_factory):
    """Three changes, then the journal keeps one: cop_update_* has to upload
    the whole table, cop_replace_* paints it."""
    rules = le.stride_edges_crafted()
    tab = Tab(rules)
    ctx, twin = (gpu_ctx_factory(stages=F | L, flags=LIVE | cg.CFG_LPM_FORCE_DIR24) for _ in range(2))
    ctx.set_route_lpm(tab.t)
    twin.set_route_lpm(tab.t)
    new = cg.prefixes([0x0A010100, 0x0A010107, 0x0A020000], [24, 32, 15], [101, 102, 103])
    for q in new:
        assert tab.t.add(int(q["ip"]), int(q["depth"]), int(q["next_hop"])) == 0
        assert tab.o.add(int(q["ip"]), int(q["depth"]), int(q["next_hop"])) == 0
    tab.t.journal_set_cap(1)
    assert twin.update_route_lpm(tab.t)["full"] == 1
    rep = ctx.replace_route_lpm(tab.t)
    assert rep["full"] == 0 and rep["n_records"] == len(cg.paint_plan(tab.t, le.FORM_NH)[0]), rep
    clean(ctx, L, tab)
    clean(twin, L, tab)
    pk, n = probes([rules, new])
    job = Job(ctx, pk, n)
    job.submit()
    ctx.sync()
    e = expect(pk, n, F | L, None, tab)
    assert_parity(*job.result(), e[0], e[1])
    # and the book is the table's generation: one more change is a patch
    assert tab.t.add(0x0A030000, 16, 104) == 0
    assert ctx.update_route_lpm(tab.t)["full"] == 0


# ---- 5. / 6. under the poll-mode kernel ------------------------------------------
class Ring:
    """A 2-slot ring of B-packet batches carrying the same frames in both slots."""

    def __init__(self, ctx, pk, B):
        self.B = B
        self.dp = ctx.alloc(2 * B * 64)
        self.dp.upload(np.concatenate([pk, pk]))
        self.dr, self.df, self.dc = ctx.alloc(2 * B * 8), ctx.alloc(2 * B * 4), ctx.alloc(2 * nseg(B) * 4 + 16)
        self.dr.fill(0xAB)
        self.ring = cg.make_ring(self.dp, 2, B, self.dr, B * 64, stride=64, fwd_idx=self.df, fwd_count=self.dc)

    def slot(self, s):
        B = self.B
        res = self.dr.download(cg.RESULT_DT, 2 * B)[s * B:(s + 1) * B]
        fwd = self.df.download(np.uint32, 2 * B)[s * B:(s + 1) * B]
        cnt = self.dc.download(np.uint32, 2 * nseg(B))[s * nseg(B):(s + 1) * nseg(B)]
        return res, seg_to_dense(fwd, cnt, B)


def test_replace_under_the_poll_mode_kernel(gpu_ctx_factory, monkeypatch):
    """fw1k in LDS, a 2-slot ring: post, wait, replace by another table object
    with every action flipped (the same LDS geometry), post, wait: slot 0 was
    served by the old table, slot 1 by the new one. A replacement that changes
    the LDS geometry returns -EBUSY and leaves the device on the table it had."""
    monkeypatch.delenv("COP_PPT", raising=False)
    rules = le.small_tables()["fw1k"][0]
    flipped = rules.copy()
    flipped["next_hop"] = np.where(rules["next_hop"] != 0, 0, 1)
    a, b, small = Tab(rules, FW1K_CFG), Tab(flipped, FW1K_CFG), Tab(le.fw_rules(le.small_tables()["halves"][0]), FW1K_CFG)
    B = 4096
    pk = le.probe_frames(le.pad_to(le.subsample(le.boundary_probes(rules), B), B)[:B])
    ctx = gpu_ctx_factory(stages=F, flags=cg.CFG_SEG_LISTS | LIVE, max_batch=B)
    ctx.set_fw_table(a.t)
    rg = Ring(ctx, pk, B)
    e0, e1 = expect(pk, B, F, a), expect(pk, B, F, b)
    assert (e0[0]["verdict"] != e1[0]["verdict"]).sum() >= 100
    with ctx.pmd_start(rg.ring) as pm:
        pm.post(1)
        pm.wait()
        before = pm.info()["launches"]
        rep = ctx.replace_fw_table(b.t)
        pm.post(1)
        pm.wait()
        info = pm.info()
        with pytest.raises(cg.CopError) as err:
            ctx.replace_fw_table(small.t)
        assert err.value.code == EBUSY
    assert rep["full"] == 0 and rep["tbl24_entries"] == 1 << 24, rep
    assert info["completed"] == 2 and info["launches"] > before, (info, before)
    assert_parity(*rg.slot(0), e0[0], e0[1])
    assert_parity(*rg.slot(1), e1[0], e1[1])
    clean(ctx, F, b)
    # with the kernel stopped the same replacement goes through
    assert ctx.replace_fw_table(small.t)["full"] == 0
    clean(ctx, F, small)


@pytest.mark.parametrize("case", ["not_live", "route_bkt"])
def test_replace_falls_back_to_the_whole_upload(gpu_ctx_factory, monkeypatch, case):
    """Where the device path does not apply the call is cop_set_* (full = 1),
    and -EBUSY under a poll-mode kernel."""
    monkeypatch.delenv("COP_PPT", raising=False)
    crafted = le.stride_edges_crafted()
    ra = np.concatenate([le.filler(), crafted]) if case == "route_bkt" else crafted
    rb = np.concatenate([pt.routes20k(), pt.crafted()]) if case == "route_bkt" else pt.crafted()
    a, b = Tab(ra), Tab(rb)
    flags = {"not_live": 0, "route_bkt": LIVE | cg.CFG_LPM_BKT}[case]
    B = 4096
    ctx = gpu_ctx_factory(stages=F | L, flags=flags | cg.CFG_SEG_LISTS, max_batch=B)
    ctx.set_route_lpm(a.t)
    assert ctx.route_form() == ("bkt" if case == "route_bkt" else "lds")
    pk, n = probes([crafted, pt.crafted()])
    pkr = le.probe_frames(le.pad_to(le.boundary_probes(crafted), B)[:B])
    rg = Ring(ctx, pkr, B)
    with ctx.pmd_start(rg.ring) as pm:
        pm.post(1)
        pm.wait()
        with pytest.raises(cg.CopError) as err:
            ctx.replace_route_lpm(b.t)
        assert err.value.code == EBUSY
    e0 = expect(pkr, B, F | L, None, a)
    assert_parity(*rg.slot(0), e0[0], e0[1])
    rep = ctx.replace_route_lpm(b.t)
    assert rep["full"] == 1 and rep["n_records"] == 0 and rep["h2d_bytes"] >= 4 << 24, rep
    # one batch with segmented forward lists (the context is CFG_SEG_LISTS for its ring)
    dp, dr, df, dc = ctx.alloc(pk.nbytes), ctx.alloc(n * 8), ctx.alloc(n * 4), ctx.alloc(nseg(n) * 4 + 16)
    dp.upload(pk)
    dr.fill(0xAB)
    ctx.submit([cg.make_batch(dp, n, dr, fwd_idx=df, fwd_count=dc)])
    ctx.sync()
    e = expect(pk, n, F | L, None, b)
    assert differ(e, expect(pk, n, F | L, None, a)) >= 100
    fwd = seg_to_dense(df.download(np.uint32, n), dc.download(np.uint32, nseg(n)), n)
    assert_parity(dr.download(cg.RESULT_DT, n), fwd, e[0], e[1])


# ---- 7. buffer reuse ---------------------------------------------------------------
def test_outgrown_tbl8_is_retired_not_freed(gpu_ctx_factory, monkeypatch):
    """A table that needs more tbl8 groups than the image has room for, with a
    job that still reads the old buffers queued in front of it; then a small
    table again; then cop_set_* and cop_destroy, which free what was retired."""
    monkeypatch.delenv("COP_PPT", raising=False)
    small, big, small2 = Tab(le.small_tables()["ends"][0]), Tab(le.lds_limit(4096)), Tab(le.small_tables()["halves"][0])
    ctx = gpu_ctx_factory(stages=F | L, flags=LIVE | cg.CFG_LPM_FORCE_DIR24, n_streams=2)
    ctx.set_route_lpm(small.t)
    pk, n = probes([small.rules, big.rules, small2.rules])
    jobs = [Job(ctx, pk, n) for _ in range(3)]
    exp = [expect(pk, n, F | L, None, t) for t in (small, big, small2)]
    jobs[0].submit()
    r1 = ctx.replace_route_lpm(big.t)
    jobs[1].submit()
    r2 = ctx.replace_route_lpm(small2.t)
    jobs[2].submit()
    ctx.sync()
    n_big = pt.form_n_ext(big.t, le.FORM_NH)
    assert n_big > 2 + 256                  # past the room a live image of `small` has
    assert r1["full"] == 0 and r1["groups_taken"] == n_big and r1["groups_released"] == 2, r1
    assert r2["full"] == 0 and r2["groups_taken"] == 0 and r2["groups_released"] == n_big, r2
    for job, e in zip(jobs, exp):
        rg, fg = job.result()
        assert_parity(rg, fg, e[0], e[1])
    clean(ctx, L, small2)
    ctx.set_route_lpm(big.t)
    clean(ctx, L, big)
    job = Job(ctx, pk, n)
    job.submit()
    ctx.sync()
    assert_parity(*job.result(), exp[1][0], exp[1][1])
    ctx.close()
