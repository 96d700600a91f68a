"""GPU: bulk lookups (cop_lookup_bulk, cop_lookup_bulk_host) and the table
audit (cop_lookup_audit).

The kernel (csrc/cop_lookup.hip) runs one stage's device table over a stream
of addresses. Its words must equal cop_lpm_lookup_words (checked against the
oracle on the host, tests/test_lookup_words.py) bit for bit: in every device
form at every prefix boundary of the tables of tests/lpm_edges.py; at every n
around the 16-byte groups, the 256-address rows and the tiles, at every
alignment, with guard bytes around the output; in place; through several
trips of the grid-stride loop; in agreement with the packet pipeline's
records; in stream order with cop_update_*; beside a poll-mode kernel.

A tile is 2,048 addresses, 1,024 in the bucketed form.
"""
import ctypes
import functools

import numpy as np
import pytest

import copgpu as cg
import lpm_edges as le
import oracle as orc
from helpers import assert_parity, gpu_run
from test_gpu_tables import MODES, ROUTE_FORM

pytestmark = pytest.mark.gpu

S, F, L = cg.STAGE_PARSE, cg.STAGE_FW, cg.STAGE_LPM
HIT, DROP = cg.LOOKUP_HIT, cg.LOOKUP_DROP
EINVAL, ENOENT = -22, -2
LARGE = ("bkt_widths", "stride_edges")
FW_LARGE = ("forced", "packed", "fwbkt")     # modes whose firewall table leaves LDS too
FW_FORM = {"forced": "dir", "packed": "dir-packed", "fwbkt": "bkt"}
GUARD = 64                                   # bytes of 0xAB before and after an output extent
SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 3 * 2048 + 259]
ALIGN = [(0, 0), (4, 0), (0, 8), (12, 12)]   # byte offsets of (ips, out) from a 16-byte boundary


@functools.lru_cache(maxsize=None)
def rule_set(name):
    small = le.small_tables()
    if name in small:
        return small[name] + (None,)
    if name == "bkt_widths":
        return le.bkt_widths(), le.RT_CFG, None
    if name == "stride_edges":
        return le.stride_edges(), le.RT_CFG, le.STRIDE_EXTRA
    assert name.startswith("lds_limit"), name
    return le.lds_limit(int(name[9:])), le.RT_CFG, None


@functools.lru_cache(maxsize=None)
def tables(name, fw):
    """(LpmTable, boundary probes) of rule set `name`, as the route table or
    (fw) as a firewall whose neighbouring rules alternate."""
    rules, cfg, extra = rule_set(name)
    if fw and name != "fw1k":
        rules = le.fw_rules(rules)
    tab = le.table(rules, cfg)
    assert tab.report.n_failed == 0, tab.report.as_dict()
    return tab, le.boundary_probes(tab, extra)


@functools.lru_cache(maxsize=None)
def probe_set(route, fw):
    p = le.subsample(np.union1d(tables(route, False)[1], tables(fw, True)[1]))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def words(name, fw, probes_of):
    """The host words of table (name, fw) over probe_set(*probes_of): computed once."""
    w = tables(name, fw)[0].lookup_words(probe_set(*probes_of), cg.LOOKUP_RULE if fw else cg.LOOKUP_NH)
    w.setflags(write=False)
    return w


def lookup(ctx, stage, ips, off_in=0, off_out=0, in_place=False):
    """ips through cop_lookup_bulk from / to device buffers at the given byte
    offsets from a 16-byte boundary, GUARD bytes of 0xAB around the output's
    extent; returns the words after checking the guards."""
    ips = np.ascontiguousarray(ips, dtype=np.uint32)
    n = len(ips)
    din = ctx.alloc(n * 4 + 2 * GUARD + 32)
    a_in = GUARD + off_in
    if n:
        din.upload(ips, a_in)
    if in_place:
        dout, a_out = din, a_in
        pre = din.download(np.uint8, a_in)
        post = din.download(np.uint8, GUARD, a_in + n * 4)
    else:
        dout = ctx.alloc(n * 4 + 2 * GUARD + 32)
        dout.fill(0xAB)
        a_out = GUARD + off_out
    ctx.lookup_bulk(stage, din.addr + a_in, n, dout.addr + a_out)
    ctx.sync()
    raw = dout.download(np.uint8, dout.nbytes)
    if in_place:
        assert np.array_equal(raw[:a_in], pre) and np.array_equal(raw[a_in + n * 4: a_in + n * 4 + GUARD], post)
    else:
        assert (raw[:a_out] == 0xAB).all(), "bytes before out were written"
        assert (raw[a_out + n * 4:] == 0xAB).all(), "bytes after out were written"
        dout.free()
    din.free()
    return raw[a_out: a_out + n * 4].view(np.uint32).copy()


def same(got, want, ips):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{bad.size} words differ, first at {bad[:8]}: ip={[hex(int(x)) for x in ips[bad[:8]]]} "
                           f"gpu={[hex(int(x)) for x in got[bad[:8]]]} host={[hex(int(x)) for x in want[bad[:8]]]}")


def load(ctx, route, fw):
    ctx.set_fw_table(tables(fw, True)[0])
    ctx.set_route_lpm(tables(route, False)[0])


# ---- 1 (and 7, first part). every form at every boundary; a clean audit ------
@pytest.mark.parametrize("route", LARGE)
@pytest.mark.parametrize("mode", list(MODES))
def test_every_form_at_every_boundary(gpu_ctx_factory, monkeypatch, route, mode):
    monkeypatch.setenv("COP_TBL8", MODES[mode][1])
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    fw = route if mode in FW_LARGE else "crafted"
    ctx = gpu_ctx_factory(stages=F | L, flags=MODES[mode][0])
    load(ctx, route, fw)
    route_form = ROUTE_FORM.get(mode, "dir") + ("-packed" if mode == "packed" else "")
    fw_form = FW_FORM[mode] if mode in FW_LARGE else "lds"
    assert ctx.lookup_form(L) == route_form and ctx.lookup_form(F) == fw_form
    assert ctx.route_form() == route_form.split("-")[0]            # the pipeline's choice for the stage
    p = probe_set(route, fw)
    assert 150000 < len(p) <= 200000
    wr, wf = words(route, False, (route, fw)), words(fw, True, (route, fw))
    assert 0.3 < ((wr & HIT) != 0).mean() < 1 and ((wf & DROP) != 0).sum() > 100 and ((wf & (HIT | DROP)) == HIT).sum() > 100
    same(lookup(ctx, L, p), wr, p)
    same(lookup(ctx, F, p), wf, p)
    # the device images answer as the host tables do
    for stage, tab, form in ((L, tables(route, False)[0], route_form), (F, tables(fw, True)[0], fw_form)):
        rep, bad = ctx.lookup_audit(stage, tab, bad_cap=8)
        assert rep["n_mismatch"] == 0 and rep["stale"] == 0 and rep["n_bad"] == 0 and len(bad) == 0, rep
        assert cg.Context.ROUTE_FORMS[rep["form"]] == form.split("-")[0]
        assert rep["n_probes"] == len(tab.audit_probes(cg.LOOKUP_RULE if stage == F else cg.LOOKUP_NH)) > 100
        assert rep["generation_device"] == 0                       # not a live context


# ---- 2. small tables ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["crafted", "empty", "halves", "ends", "fw1k", "lds_limit4096"])
def test_small_tables_in_lds(gpu_ctx_factory, monkeypatch, name):
    monkeypatch.delenv("COP_TBL8", raising=False)
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    ctx = gpu_ctx_factory(stages=S)                                # neither stage is in cfg.stages
    load(ctx, name, name)
    assert ctx.lookup_form(L) == "lds" and ctx.lookup_form(F) == "lds"
    p = probe_set(name, name)
    wr, wf = words(name, False, (name, name)), words(name, True, (name, name))
    if name == "empty":
        assert not wr.any() and not wf.any()
    if name == "ends":
        assert p[0] == 0 and p[-1] == 0xFFFFFFFF and wr[0] == (5 | HIT) and wr[-1] == (6 | HIT)
    if name == "lds_limit4096":
        assert tables(name, False)[0].report.n_intervals == le.IVT_MAX
    same(lookup(ctx, L, p), wr, p)
    same(lookup(ctx, F, p), wf, p)
    assert ctx.lookup_audit(L, tables(name, False)[0])[0]["n_mismatch"] == 0


def test_one_interval_past_the_lds_limit(gpu_ctx_factory, monkeypatch):
    monkeypatch.delenv("COP_TBL8", raising=False)
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    ctx = gpu_ctx_factory(stages=F | L)
    load(ctx, "lds_limit4097", "crafted")
    assert tables("lds_limit4097", False)[0].report.n_intervals == le.IVT_MAX + 2
    assert ctx.lookup_form(L) == "dir" and ctx.lookup_form(F) == "lds"
    p = probe_set("lds_limit4097", "crafted")
    same(lookup(ctx, L, p), words("lds_limit4097", False, ("lds_limit4097", "crafted")), p)


# ---- 3. sizes, alignment, bounds -----------------------------------------------------
SHAPES = {"lds": ("crafted", 0, 2048), "dir": ("stride_edges", 0, 2048), "bkt": ("bkt_widths", cg.CFG_LPM_BKT, 1024)}


@pytest.mark.parametrize("form", list(SHAPES))
def test_sizes_alignment_bounds(gpu_ctx_factory, monkeypatch, form):
    name, flags, tile = SHAPES[form]
    monkeypatch.setenv("COP_TBL8", "plain")
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    ctx = gpu_ctx_factory(stages=L, flags=flags)
    tab, probes = tables(name, False)
    ctx.set_route_lpm(tab)
    assert ctx.lookup_form(L) == form
    nmax = max(SIZES)
    # the crafted rules' edges first (hits and misses side by side), then the rest
    crafted = le.boundary_probes(le.bkt_widths_crafted() if name == "bkt_widths" else le.stride_edges_crafted())
    ips = le.pad_to(np.concatenate([crafted, probes]), nmax)[:nmax]
    want = tab.lookup_words(ips, cg.LOOKUP_NH)
    assert 0.2 < ((want[:256] & HIT) != 0).mean() < 1
    for n in SIZES:
        for off_in, off_out in ALIGN:
            same(lookup(ctx, L, ips[:n], off_in, off_out), want[:n], ips[:n])
    # in place, on both paths (16-byte aligned and not)
    for n in (1, 5, 257, 2049, nmax):
        for off in (0, 4):
            same(lookup(ctx, L, ips[:n], off, in_place=True), want[:n], ips[:n])
    # any other overlap is refused, and writes nothing
    buf = ctx.alloc(4096)
    buf.fill(0xAB)
    for d_in, d_out, n in ((0, 4, 2), (16, 0, 100), (0, 1020, 256)):
        with pytest.raises(cg.CopError) as e:
            ctx.lookup_bulk(L, buf.addr + d_in, n, buf.addr + d_out)
        assert e.value.code == EINVAL and "overlap" in str(e.value)
    ctx.lookup_bulk(L, buf.addr, 256, buf.addr + 1024)              # adjacent extents are fine
    ctx.sync()
    assert (buf.download(np.uint8, 2048, 2048) == 0xAB).all()


@pytest.mark.parametrize("form", list(SHAPES))
def test_grid_stride_trips(gpu_ctx_factory, monkeypatch, form):
    """$COP_LOOKUP_GRID=3 with 7 tiles + 259 addresses: every workgroup takes
    two or three trips, the last tile is partial."""
    name, flags, tile = SHAPES[form]
    monkeypatch.setenv("COP_TBL8", "plain")
    monkeypatch.setenv("COP_LOOKUP_GRID", "3")
    ctx = gpu_ctx_factory(stages=L, flags=flags)
    tab, probes = tables(name, False)
    ctx.set_route_lpm(tab)
    assert ctx.lookup_form(L) == form
    n = 7 * tile + 259
    ips = le.pad_to(probes, n)[:n] if len(probes) < n else le.subsample(probes, n)[:n]
    assert len(ips) == n
    want = tab.lookup_words(ips, cg.LOOKUP_NH)
    for off_in, off_out in ((0, 0), (4, 8)):
        same(lookup(ctx, L, ips, off_in, off_out), want, ips)


# ---- 4. agreement with the pipeline ----------------------------------------------------
def test_agreement_with_the_pipeline(gpu_ctx_factory, monkeypatch):
    monkeypatch.setenv("COP_TBL8", "plain")
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    ctx = gpu_ctx_factory(stages=F | L)
    load(ctx, "stride_edges", "crafted")
    p = probe_set("stride_edges", "crafted")
    src, dst = p, np.ascontiguousarray(p[::-1])
    res, _, _ = gpu_run(ctx, le.probe_frames(src, dst), len(p), batches=1)
    wr, wf = lookup(ctx, L, dst), lookup(ctx, F, src)
    assert np.array_equal(res["route_nh"], wr & 0x00FFFFFF)
    assert np.array_equal((res["flags"] & cg.FLAG_ROUTE_HIT) != 0, (wr & HIT) != 0)
    assert np.array_equal((res["flags"] & cg.FLAG_FW_HIT) != 0, (wf & HIT) != 0)
    assert np.isin(res["verdict"], (cg.FORWARD, cg.DROP_FW)).all()
    assert np.array_equal(res["verdict"] == cg.DROP_FW, (wf & DROP) != 0)
    assert ((wf & DROP) != 0).sum() > 100 and ((wr & HIT) != 0).sum() > 1000


# ---- 5. ordering with live updates ---------------------------------------------------------
def live_script(rules):
    """Adds (a /24, a /32 inside it, a /25 beside it, a /8 over crafted
    rules), overwrites (actions flipped) and deletes of held rules."""
    ops = [("add", 0x0A010100, 24, 0x111), ("add", 0x0A010107, 32, 0), ("add", 0x0A010280, 25, 0x222),
           ("add", 0x0C000000, 8, 0x333), ("add", 0x0A010107, 32, 0x444)]
    for k in (0, 1, 7, 20, 21):
        r = rules[k]
        ops.append(("add", int(r["ip"]), int(r["depth"]), 0 if r["next_hop"] else 0x555))
    for k in (2, 3, 30, 31, 50):
        ops.append(("del", int(rules[k]["ip"]), int(rules[k]["depth"])))
    return ops


@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("form", ["dir", "lds"])
def test_ordering_with_live_updates(gpu_ctx_factory, monkeypatch, form, n_streams):
    monkeypatch.delenv("COP_TBL8", raising=False)
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    flags = cg.CFG_LIVE_TABLES
    if form == "dir":
        flags |= cg.CFG_FW_FORCE_DIR24 | cg.CFG_LPM_FORCE_DIR24 | cg.CFG_RULE_COUNTERS
    rules = le.stride_edges_crafted()
    trt, tfw = le.table(rules), le.table(le.fw_rules(rules))
    ops = live_script(trt.rules())
    touched = cg.prefixes([o[1] for o in ops], [o[2] for o in ops], [1] * len(ops))
    p = le.pad_to(np.union1d(le.boundary_probes(trt), le.boundary_probes(touched)), 3 * 2048 + 259)
    ctx = gpu_ctx_factory(stages=F | L, flags=flags, n_streams=n_streams)
    ctx.set_fw_table(tfw)
    ctx.set_route_lpm(trt)
    assert ctx.lookup_form(L) == form and ctx.lookup_form(F) == form
    # some pipeline traffic first, so the counters are not zero
    gpu_run(ctx, le.probe_frames(p[:4096]), 4096, batches=1)
    c0 = ctx.counters()
    assert c0["rx"] == 4096
    din = ctx.alloc(len(p) * 4)
    din.upload(p)
    bufs = {(st, g): ctx.alloc(len(p) * 4) for st in (F, L) for g in "ABCD"}
    for b in bufs.values():
        b.fill(0xAB)
    host = {}

    def capture(g):
        host[(F, g)], host[(L, g)] = tfw.lookup_words(p, cg.LOOKUP_RULE), trt.lookup_words(p, cg.LOOKUP_NH)

    def queue(g):
        for st in (F, L):
            ctx.lookup_bulk(st, din, len(p), bufs[(st, g)])

    capture("A")
    queue("A")
    for t in (tfw, trt):
        for op in ops:
            assert (t.add(*op[1:]) if op[0] == "add" else t.delete(*op[1:])) == 0, op
    reps = [ctx.update_fw_table(tfw), ctx.update_route_lpm(trt)]
    capture("B")
    queue("B")
    assert tfw.delete_all() == 0 and trt.delete_all() == 0
    reps += [ctx.update_fw_table(tfw), ctx.update_route_lpm(trt)]
    capture("C")
    queue("C")
    ctx.sync()                                                     # the one sync
    assert all(r["full"] == 0 and r["n_changes"] > 0 for r in reps), reps
    assert ctx.lookup_form(L) == form
    for st in (F, L):
        assert (host[(st, "A")] != host[(st, "B")]).sum() >= 20   # an update that did nothing would show
        assert host[(st, "B")].any() and not host[(st, "C")].any()
        for g in "ABC":
            same(bufs[(st, g)].download(np.uint32, len(p)), host[(st, g)], p)
    # lookups that hit, on tables with rules again: no counter moves
    for t in (tfw, trt):
        assert t.add(0x0B000000, 8, 1) == 0 and t.add(0x0D000100, 24, 0) == 0
    ctx.update_fw_table(tfw)
    ctx.update_route_lpm(trt)
    capture("D")
    queue("D")
    ctx.sync()
    for st in (F, L):
        assert (host[(st, "D")] & HIT).any()
        same(bufs[(st, "D")].download(np.uint32, len(p)), host[(st, "D")], p)
    assert ctx.counters() == c0
    if form == "dir":
        assert not ctx.rule_counters().any()                       # zeroed by delete_all's update, untouched since
    for st, t in ((F, tfw), (L, trt)):
        rep, _ = ctx.lookup_audit(st, t)
        assert rep["n_mismatch"] == 0 and rep["stale"] == 0 and rep["generation_device"] == t.generation, rep


# ---- 6. beside the poll-mode kernel ----------------------------------------------------------
def test_beside_the_poll_mode_kernel(gpu_ctx_factory, monkeypatch):
    monkeypatch.delenv("COP_PPT", raising=False)
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    t = cg.LpmTable(rules, 1024, 24, True)
    ofw = orc.OracleLpm(1024, 24)
    ofw.setup(rules["ip"], rules["depth"], rules["next_hop"])
    B = 4096
    p = le.pad_to(le.boundary_probes(t), 2 * B)[:2 * B]
    pk = le.probe_frames(p)
    ctx = gpu_ctx_factory(stages=F, max_batch=B)
    ctx.set_fw_table(t)
    dp = ctx.alloc(2 * B * 64)
    dp.upload(pk)
    dr, df, dc = ctx.alloc(2 * B * 8), ctx.alloc(2 * B * 4), ctx.alloc(64)
    dr.fill(0xAB)
    ring = cg.make_ring(dp, 2, B, dr, B * 64, stride=64, fwd_idx=df, fwd_count=dc)
    din = ctx.alloc(len(p) * 4)
    din.upload(p)
    # the words go to mapped host memory: read below without any call that could wait for the GPU
    hptr, dptr = ctypes.c_void_p(), ctypes.c_void_p()
    assert cg.lib().cop_host_alloc_mapped(ctx.handle, len(p) * 4, ctypes.byref(hptr), ctypes.byref(dptr)) == 0
    hout = np.frombuffer((ctypes.c_uint8 * (len(p) * 4)).from_address(hptr.value), dtype=np.uint32)
    hout[:] = 0xABABABAB
    want = t.lookup_words(p, cg.LOOKUP_RULE)
    try:
        with ctx.pmd_start(ring) as pm:
            pm.post(1)
            pm.wait()
            i0 = pm.info()
            assert i0["state"] == 0 and i0["completed"] == 1, i0    # running
            ctx.lookup_bulk(F, din, len(p), dptr.value)
            got = hout.copy()                                      # valid on return
            pm.post(1)
            pm.wait()
            i1 = pm.info()
        same(got, want, p)
        assert i1["state"] == 0 and i1["completed"] == 2 and i1["launches"] == i0["launches"] + 1, (i0, i1)
        res = dr.download(cg.RESULT_DT, 2 * B)
        fwd = df.download(np.uint32, 2 * B)
        cnt = dc.download(np.uint32, 2)
        for s in range(2):
            ro, fo, _ = orc.process(pk[s * B * 64:(s + 1) * B * 64], B, stages=F, fw=ofw)
            assert_parity(res[s * B:(s + 1) * B], fwd[s * B: s * B + int(cnt[s])], ro, fo)
    finally:
        del hout
        cg.lib().cop_host_free_pinned(ctx.handle, hptr)


# ---- 7. audit ------------------------------------------------------------------------------------
def test_audit_finds_what_the_host_changed(gpu_ctx_factory, monkeypatch):
    monkeypatch.delenv("COP_TBL8", raising=False)
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    rules = le.stride_edges_crafted()
    t = le.table(rules)
    ctx = gpu_ctx_factory(stages=L, flags=cg.CFG_LIVE_TABLES | cg.CFG_LPM_FORCE_DIR24)
    ctx.set_route_lpm(t)
    assert ctx.lookup_form(L) == "dir"
    # 500 random live mutations, one update
    rng = np.random.default_rng(0xA0D17)
    held = [(int(r["ip"]), int(r["depth"])) for r in t.rules()]
    for _ in range(500):
        k = int(rng.integers(0, 3))
        if k == 0 and len(held) > 50:
            ip, d = held.pop(int(rng.integers(0, len(held))))
            assert t.delete(ip, d) == 0
        elif k == 1:
            ip, d = held[int(rng.integers(0, len(held)))]
            assert t.add(ip, d, int(rng.integers(1, 1 << 24))) == 0
        else:
            d = int(rng.integers(8, 33))
            ip = (0x0A000000 | int(rng.integers(0, 1 << 22))) & ((0xFFFFFFFF << (32 - d)) & 0xFFFFFFFF)
            assert t.add(ip, d, int(rng.integers(1, 1 << 24))) == 0
            if (ip, d) not in held:
                held.append((ip, d))
    assert ctx.lookup_audit(L, t)[0]["stale"] == 1                 # mutated, not yet applied
    rep = ctx.update_route_lpm(t)
    assert rep["full"] == 0 and rep["n_changes"] == 500
    rep, bad = ctx.lookup_audit(L, t, bad_cap=16)
    assert rep["n_mismatch"] == 0 and rep["stale"] == 0 and len(bad) == 0, rep
    assert rep["generation_table"] == rep["generation_device"] == t.generation == 500
    # one /24 with an unused next hop, on the host only
    lo, hi, nh = 0x0E010200, 0x0E0102FF, 0x00ABCDE
    ends = np.array([lo, hi], np.uint32)
    before = t.lookup_words(ends)
    assert t.add(lo, 24, nh) == 0
    after = t.lookup_words(ends)
    assert (before != after).all() and (after == (nh | HIT)).all()
    rep, bad = ctx.lookup_audit(L, t, bad_cap=16)
    assert rep["stale"] == 1 and rep["n_mismatch"] >= 2 and rep["n_bad"] == len(bad) == min(16, rep["n_mismatch"]), rep
    assert rep["generation_table"] == 501 and rep["generation_device"] == 500
    assert ((bad >= lo) & (bad <= hi)).all() and (np.diff(bad.astype(np.int64)) > 0).all()
    assert {lo, hi} <= set(bad.tolist())
    assert rep["first_ip"] == bad[0] == lo and rep["first_host"] == (nh | HIT) and rep["first_device"] == before[0]
    # each reported address genuinely differs between the two host states
    assert t.delete(lo, 24) == 0
    old = t.lookup_words(bad)
    assert t.add(lo, 24, nh) == 0
    assert (t.lookup_words(bad) != old).all()
    assert ctx.lookup_audit(L, t)[0]["stale"] == 1
    rep2 = ctx.update_route_lpm(t)
    assert rep2["full"] == 0
    rep, bad = ctx.lookup_audit(L, t, bad_cap=16)
    assert rep["n_mismatch"] == 0 and rep["stale"] == 0 and len(bad) == 0, rep
    # against a different table object
    other = le.table(np.concatenate([rules, cg.prefixes([0x0F000000], [8], [77])]))
    rep, bad = ctx.lookup_audit(L, other, bad_cap=1 << 16)
    assert rep["stale"] == 1 and rep["n_mismatch"] > 0 and rep["n_bad"] == rep["n_mismatch"]
    dev = ctx.lookup_bulk_host(L, bad)
    assert (dev != other.lookup_words(bad)).all() and np.array_equal(dev, t.lookup_words(bad))
    assert rep["first_ip"] == bad[0] and rep["first_device"] == dev[0]
    assert 0x0F000000 in bad.tolist() and 0x0FFFFFFF in bad.tolist()


# ---- 8. refusals ------------------------------------------------------------------------------------
def test_refusals(gpu_ctx_factory, monkeypatch):
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    ctx = gpu_ctx_factory(stages=F | L)
    buf = ctx.alloc(4096)
    buf.fill(0xAB)

    def refused(code, word, stage, a_in=0, a_out=2048, n=16):
        with pytest.raises(cg.CopError) as e:
            ctx.lookup_bulk(stage, buf.addr + a_in, n, buf.addr + a_out)
        assert e.value.code == code and word in str(e.value), str(e.value)

    for stage in (0, F | L, S, 0x8, F | 0x10):
        refused(EINVAL, "stage", stage)
    refused(ENOENT, "no table", F)                                 # only cop_create's empty images so far
    refused(ENOENT, "no table", L)
    with pytest.raises(cg.CopError) as e:
        ctx.lookup_form(L)
    assert e.value.code == ENOENT
    with pytest.raises(cg.CopError) as e:
        ctx.lookup_bulk_host(L, np.zeros(4, np.uint32))
    assert e.value.code == ENOENT
    t = tables("crafted", False)[0]
    with pytest.raises(cg.CopError) as e:
        ctx.lookup_audit(L, t)
    assert e.value.code == ENOENT
    ctx.set_route_lpm(t)
    refused(ENOENT, "no table", F)                                 # the other stage still has none
    for a_in, a_out in ((1, 2048), (2, 2048), (0, 2049), (3, 2051)):
        refused(EINVAL, "aligned", L, a_in, a_out)
    refused(EINVAL, "stage", F | L)
    ctx.lookup_bulk(L, buf.addr, 0, buf.addr + 2048)               # n = 0: nothing happens
    ctx.lookup_bulk(L, 0, 0, 0)
    ctx.sync()
    assert (buf.download(np.uint8, 4096) == 0xAB).all()
    assert len(ctx.lookup_bulk_host(L, np.zeros(0, np.uint32))) == 0


# ---- 9. host arrays ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [1, 2])
def test_lookup_bulk_host(gpu_ctx_factory, monkeypatch, n_streams):
    monkeypatch.setenv("COP_TBL8", "plain")
    monkeypatch.delenv("COP_LOOKUP_GRID", raising=False)
    ctx = gpu_ctx_factory(stages=L, n_streams=n_streams)
    tab, probes = tables("stride_edges", False)
    ctx.set_route_lpm(tab)
    n = 3 * cg.LOOKUP_STAGE_WORDS + 17
    rng = np.random.default_rng(0xB01C)
    ips = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ips[:len(probes)] = probes                                     # chunk 0 starts on the boundaries
    ips[-17:] = probes[-17:]                                       # the tail chunk
    got = ctx.lookup_bulk_host(L, ips)
    same(got, tab.lookup_words(ips), ips)
    # in place on the host side too
    a = ips[:5000].copy()
    assert cg.lib().cop_lookup_bulk_host(ctx.handle, L, a.ctypes.data, len(a), a.ctypes.data) == 0
    same(a, got[:5000], ips[:5000])
