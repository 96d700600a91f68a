"""GPU: cop_neigh_* / cop_fwd_check / cop_fwd_rewrite (csrc/cop_fwd.hip), the L3
forward step on the device.

The cases are fwd_cases', which test_fwd_host.py holds against the host mirror:
frames with random bytes everywhere but the fields set on purpose, a
prescribed class per packet, every output between 0xAB guards. All arrays of a
call sit in one device buffer whose whole image is compared afterwards, so only
outputs may differ; the table comes back through its device pointer and must be
what cop_neigh_set put there.
"""
import ctypes

import numpy as np
import pytest

import copgpu as cg
import fwd_cases as fc
import sketch_cases as sc
import tx_cases as tc
import verdict_patterns as vp

pytestmark = pytest.mark.gpu

S, F, L = vp.S, vp.F, vp.L
EINVAL = -22
FLAGS = {"dense": 0, "seg": cg.CFG_SEG_LISTS, "demux": cg.CFG_DEMUX_PORTS}
KP = {"dense": 1, "seg": 1, "demux": 5}
LAYOUTS = list(fc.LAYOUTS)
PAD = fc.PAD
VERIFY = cg.FWD_VERIFY_CSUM


def ctx_of(factory, form="dense", **kw):
    return factory(stages=S, n_ports=5, flags=FLAGS[form], **kw)


def neigh_of(ctx, table):
    ng = ctx.neigh(len(table))
    ng.set(0, table)
    return ng


def table_on_device(ctx, ng):
    dptr, n = ng.device_ptr()
    out = np.zeros(n, dtype=cg.NEIGH_DT)
    assert cg.lib().cop_memcpy_d2h(ctx.handle, out.ctypes.data, ctypes.c_void_p(dptr), out.nbytes) == 0
    return out


def run(ctx, cases, what, times=1):
    """One call per 32 cases that share a table and a config; the whole image compared."""
    ng = neigh_of(ctx, cases[0].table)
    for lo in range(0, len(cases), 32):
        part = cases[lo:lo + 32]
        p = sc.Pack(ctx, part)
        bs, ds, ts, rs = fc.pack_descs(p)
        for _ in range(times):
            if what == "check":
                ctx.fwd_check(ng, part[0].cfg(), bs, ds)
            else:
                ctx.fwd_rewrite(ng, part[0].cfg(), bs, ts, rs)
        ctx.sync()
        for c in part:
            c.expect_check() if what == "check" else c.expect_rewrite(times)
        p.check(outputs=range(len(part)))
    assert np.array_equal(table_on_device(ctx, ng), cases[0].table)      # the table is not written
    ng.destroy()


def groups(cases):
    """Cases grouped by what a call shares: the flags, miss_nh and the (default) table."""
    out = {}
    for c in cases:
        out.setdefault((c.flags, c.miss_nh, c.n_entries), []).append(c)
    return out.values()


# ---- 1. check, every list form ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FLAGS))
@pytest.mark.parametrize("n", sc.NS)
def test_check_every_list_form(gpu_ctx_factory, n, form):
    ctx = ctx_of(gpu_ctx_factory, form)
    layout = LAYOUTS[sc.NS.index(n) % 4]
    cases = []
    for j, (name, fwd) in enumerate(tc.masks(n).items()):
        cases.append(fc.FwdCase(n, layout, form, fwd, KP[form], seed=8, flags=VERIFY * (j % 2), miss=fc.MISS[j % 3],
                                exc=j % 4 != 3))
    for g in groups(cases):
        run(ctx, g, "check")
    c = ctx.counters()
    assert c["rx"] == 0 and c["forward"] == 0, c                         # no pipeline counter is touched


# ---- 2. check, many chunks and clamps ---------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FLAGS))
def test_check_many_chunks_and_clamps(gpu_ctx_factory, form):
    ctx = ctx_of(gpu_ctx_factory, form)
    n, K = vp.LONG_N, KP[form]
    a = fc.FwdCase(n, "s64", form, vp.patterns(n, 256)["alt_tile"], K, seed=1, flags=VERIFY)
    b = fc.FwdCase(n, "imix", form, vp.patterns(n, 256)["all"], K, seed=2, flags=VERIFY)
    c = fc.FwdCase(600, "s128", form, vp.patterns(600, 256)["all"], K, seed=3, flags=VERIFY)
    c.inputs["counts"][:] = 0xFFFFFFF0                                   # counts above what the layout holds
    junk = c.inputs["idx"] == tc.JUNK                                    # junk past the counts, now inside them
    c.inputs["idx"][junk] = 600 + 5 + np.arange(junk.sum())
    c.inputs["idx"][::7] += 600                                          # indices >= n
    run(ctx, [a, fc.FwdCase(0, "s64", form, K=K, flags=VERIFY), b, c], "check")
    assert 0 < a.check_status()[0][0] < a.inputs["counts"].sum()


# ---- 3. rewrite, forms x layouts -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("form", list(FLAGS))
def test_rewrite_forms_layouts_and_capacity_cuts(gpu_ctx_factory, form, layout):
    """W below the list's length: frames at or past W, their port words and all guards stay; port[] is exact."""
    ctx = ctx_of(gpu_ctx_factory, form)
    n, K = 700, KP[form]
    cases = []
    for j, (flags, miss) in enumerate(((0, "valid"), (VERIFY, "invalid"), (VERIFY, "none"))):
        cases.append(fc.FwdCase(n, layout, form, vp.patterns(n, 256)["bern_63_64"], K, seed=j, flags=flags,
                                miss=miss).with_tx(port=j != 1))
    if form == "dense":
        fwd = vp.patterns(n, 256)["all"]
        for name, c in tc.cap_cases(lambda caps: fc.FwdCase(n, layout, form, fwd, seed=5).with_tx(caps).tx):
            cases.append(fc.FwdCase(n, layout, form, fwd, seed=5).with_tx(c.caps))
    else:
        full = fc.FwdCase(n, layout, form, None, K, seed=6).with_tx().tx
        caps = [(int(e["status"][PAD // 4 + 1]) // 2 & ~15, 10_000) for e in full.expect]
        cut = fc.FwdCase(n, layout, form, None, K, seed=6).with_tx(caps)
        assert 0 < cut.expect[0]["tx_status0"][PAD // 4] < len(cut.true_lists[0])
        few = fc.FwdCase(n, layout, form, None, K, seed=6).with_tx([(1 << 20, 77 + q) for q in range(len(caps))])
        cases += [cut, few]
    for small in (0, 1, 257):
        cases.append(fc.FwdCase(small, layout, form, None, K, seed=9).with_tx())
    for g in groups(cases):
        run(ctx, g, "rewrite")
    st = cases[0].expect[0]["rw_status0"][PAD // 4:PAD // 4 + 4]
    assert st[0] > 0 and st[1] > 0, st


def test_rewrite_twice_and_without_records(gpu_ctx_factory):
    ctx = ctx_of(gpu_ctx_factory)
    d = fc.FwdCase(300, "imix", "dense", seed=8).with_tx()
    run(ctx, [d], "rewrite", times=2)                                    # TTL 2 frames are TTL class the second time
    assert d.expect[0]["rw_status0"][PAD // 4 + 2] > 0
    run(ctx, [fc.FwdCase(300, "s64", "dense", seed=7, with_results=False).with_tx()], "rewrite")


# ---- 4. checksum corners ------------------------------------------------------------------------------------
def test_checksum_corners_on_the_device(gpu_ctx_factory):
    """Every TTL 2..255, plain and with either checksum corner; random (invalid) checksums without VERIFY."""
    ctx = ctx_of(gpu_ctx_factory)
    rng = np.random.default_rng(4)
    n = 254 * 3
    table = fc.make_table(4)
    for flags, valid in ((VERIFY, True), (0, False)):
        c = fc.FwdCase(n, "s64", "dense", seed=4, flags=flags, table=table, n_entries=4)
        pk, s = c.inputs["pkts"], c.starts
        ttl = (2 + np.arange(n) // 3).astype(np.uint8)
        fc.set_valid_header(pk, s, ttl, np.arange(n) % 3)
        if not valid:
            pk[s + 24], pk[s + 25] = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
        c.inputs["results"]["flags"] = cg.FLAG_ROUTE_HIT
        c.inputs["results"]["route_nh"] = 2
        c.with_tx()
        run(ctx, [c], "rewrite")
        o = PAD // 4
        assert c.expect[0]["rw_status0"][o:o + 4].tolist() == [n, 0, 0, 0]
        fr = c.expect[0]["tx_frames0"][PAD:PAD + 64 * n].reshape(n, 64)
        assert np.array_equal(fr[:, 22], ttl - 1)
        if valid:                                                        # eqn 3 is the full recompute
            new = (fr[:, 24].astype(np.int64) << 8) | fr[:, 25]
            assert np.array_equal(new, fc.csum_full(fr[:, :34]))
            assert (new[1::3] == 0).all()                                # where HC + 0x0100 would give 0xFFFF


# ---- 5. table edges ------------------------------------------------------------------------------------------
def edge_case(table, n_entries, valid, invalid, miss="none", n=200):
    return fc.FwdCase(n, "s64", "dense", seed=3, flags=VERIFY, miss=miss, n_entries=n_entries, table=table,
                      valid_nh=valid, invalid_nh=invalid)


def test_table_edges(gpu_ctx_factory):
    ctx = ctx_of(gpu_ctx_factory)
    t = fc.make_table(10)
    t["flags"][9] |= 1
    t["flags"][4] &= 0xFFFE                                              # an invalid entry amid valid ones
    c = edge_case(t, 10, [9, 0, 8], [10, 4, 11, 0xFFFFFF])              # n_entries - 1 and n_entries
    run(ctx, [c], "check")
    assert c.check_status()[0][3] > 0
    run(ctx, [edge_case(t, 10, [9, 0, 8], [10, 4, 11, 0xFFFFFF]).with_tx()], "rewrite")
    one = fc.make_table(1)
    run(ctx, [edge_case(one, 1, [0], [1, 2, 0xFFFFFF], miss="valid")], "check")
    run(ctx, [edge_case(one, 1, [0], [1, 2, 0xFFFFFF], miss="valid").with_tx()], "rewrite")


def test_neigh_set_of_sub_ranges(gpu_ctx_factory):
    ctx = ctx_of(gpu_ctx_factory)
    t = fc.make_table(300, seed=2)
    ng = ctx.neigh(300)
    assert not table_on_device(ctx, ng).view(np.uint8).any()             # zero, so invalid, at creation
    ng.set(7, t[7:200])
    ng.set(299, t[299:])
    ng.set(0, t[:1])
    ng.set(300, t[:0])                                                   # an empty range at the end
    want = np.zeros(300, dtype=cg.NEIGH_DT)
    want[7:200], want[299], want[0] = t[7:200], t[299], t[0]
    assert np.array_equal(table_on_device(ctx, ng), want)
    for first, count in ((300, 1), (0, 301), (0xFFFFFFFF, 2), (5, 0xFFFFFFFF)):
        with pytest.raises(cg.CopError) as e:
            ng.set(first, t, count)
        assert e.value.code == EINVAL
    with pytest.raises(cg.CopError) as e:
        ng.set(0, None, 4)
    assert e.value.code == EINVAL
    assert np.array_equal(table_on_device(ctx, ng), want)
    c = fc.FwdCase(300, "s64", "dense", seed=5, table=want, n_entries=300, valid_nh=[0, 8, 198, 10],
                   invalid_nh=[200, 298, 7, 300], miss="none")
    p = sc.Pack(ctx, [c])
    bs, ds, _, _ = fc.pack_descs(p)
    ctx.fwd_check(ng, c.cfg(), bs, ds)
    ctx.sync()
    c.expect_check()
    p.check(outputs=[0])
    for n_entries in (0, (1 << 24) + 1):
        with pytest.raises(cg.CopError) as e:
            ctx.neigh(n_entries)
        assert e.value.code == EINVAL


def test_the_largest_table(gpu_ctx_factory):
    """n_entries = 1 << 24: next hop 0xFFFFFF is the last entry."""
    ctx = ctx_of(gpu_ctx_factory)
    ne = 1 << 24
    ng = ctx.neigh(ne)
    ends = fc.make_table(4, seed=9)
    ends["flags"] = (ends["flags"] & 0xFFFE) | (1, 0, 0, 1)
    ng.set(0, ends[:2])
    ng.set(ne - 2, ends[2:])

    class Sparse:                                                        # the table the restatement reads
        def __getitem__(self, key):
            if isinstance(key, str):
                return Sparse.Field(key)
            i = np.asarray(key)
            return ends[np.where(i >= ne - 2, i - (ne - 4), np.minimum(i, 1))]

        class Field:
            def __init__(self, name):
                self.name = name

            def __getitem__(self, i):
                i = np.asarray(i)
                v = ends[self.name][np.where(i >= ne - 2, i - (ne - 4), np.minimum(i, 1))]
                return np.where((i < 2) | (i >= ne - 2), v, 0)

    c = fc.FwdCase(300, "s64", "dense", seed=6, flags=VERIFY, miss="none", n_entries=ne, table=Sparse(),
                   valid_nh=[0xFFFFFF, 0], invalid_nh=[0xFFFFFE, 1, 12345]).with_tx()
    p = sc.Pack(ctx, [c])
    bs, ds, ts, rs = fc.pack_descs(p)
    ctx.fwd_check(ng, c.cfg(), bs, ds)
    ctx.fwd_rewrite(ng, c.cfg(), bs, ts, rs)
    ctx.sync()
    c.expect_check()
    c.expect_rewrite()
    p.check(outputs=[0])
    assert c.expect[0]["rw_status0"][PAD // 4] > 0 and c.check_status()[0][3] > 0


# ---- 6. the whole chain with no sync -------------------------------------------------------------------------
def pipeline_ctx(factory, form, **kw):
    ctx = factory(stages=S | F | L, n_ports=5, flags=FLAGS[form], routing_table=vp.routing_table(5), **kw)
    ctx.set_fw_table(cg.LpmTable(vp.fw_rules(), *vp.FW_CFG))
    ctx.set_route_lpm(cg.LpmTable(vp.route_rules(), 1 << 20, 1 << 16, False))
    return ctx


def l3_frames(n, mask, K=5):
    """Prescribed pipeline frames (verdict_patterns.frames) with option-less headers, TTLs 0..255 and valid checksums."""
    fwd = vp.patterns(n, 256)[mask]
    ports = vp.port_layouts(n, 256, K)["wave"]
    pk, rec, cnt = vp.frames(vp.classes_of(mask, fwd), ports, vp.route_hit_mask(n), S | F | L)
    f = pk.reshape(n, 64)
    v4 = (f[:, 14] >> 4) == 4
    f[v4, 14] = 0x45
    f[:, 22] = np.array([64, 2, 1, 255, 0, 3, 128], dtype=np.uint8)[np.arange(n) % 7]
    hc = fc.csum_full(f[:, :34])
    f[:, 24], f[:, 25] = hc >> 8, hc & 0xFF
    return pk, rec, cnt, fwd, ports


def chain_table():
    t = fc.make_table(1 << 20, seed=1)
    t["flags"][vp.ROUTE_NH[0]] |= 1
    t["flags"][vp.ROUTE_NH[1]] |= 1
    return t


@pytest.mark.parametrize("form", list(FLAGS))
def test_submit_check_gather_rewrite_seal_without_sync(gpu_ctx_factory, form):
    ctx = pipeline_ctx(gpu_ctx_factory, form, n_streams=2)
    n, K = 1027, KP[form]
    nl, cw = (K if form == "demux" else 1), max(vp.nseg(n), K)
    pk, rec, cnt, fwd, ports = l3_frames(n, "bern_63_64")
    table = chain_table()
    ng = neigh_of(ctx, table)
    cfg = cg.fwd_config(VERIFY, 5)                                       # entry 5 is invalid: route misses are NO_NEIGH
    key = cg.aead_key(bytes(range(32)), b"\x01\x02\x03\x04")
    cap_frames, cap_bytes = n, n * 64
    # name -> (bytes, per list?)
    shapes = {"res": n * 8, "idx": n * 4 * nl, "cnt": 4 * cw, "oidx": n * 4 * nl, "ocnt": 4 * cw, "eidx": n * 4 * nl,
              "ecnt": 4 * cw, "cst": 16 * nl}
    per = {"frames": cap_bytes, "off": 4 * cap_frames, "len": 4 * cap_frames, "txst": 16, "port": 4 * cap_frames,
           "rwst": 16, "tags": 16 * cap_frames, "aest": 16}
    for q in range(nl):
        shapes.update({f"{k}{q}": v for k, v in per.items()})
    dev = {k: ctx.alloc(v) for k, v in shapes.items()}
    host = {k: tc.aligned(v, 0xAB) for k, v in shapes.items()}
    for d in dev.values():
        d.fill(0xAB)
    d_pk = ctx.alloc(n * 64)
    d_pk.upload(pk)
    h_pk = tc.aligned(n * 64)
    h_pk[:] = pk

    def descs(a, pkts):
        batch = cg.make_batch(pkts, n, a("res"), 64, fwd_idx=a("idx"), fwd_count=a("cnt"))
        chk = cg.make_fwd_check(a("oidx"), a("ocnt"), a("cst"), exc_idx=a("eidx"), exc_count=a("ecnt"))
        filtered = cg.make_batch(pkts, n, a("res"), 64, fwd_idx=a("oidx"), fwd_count=a("ocnt"))
        tx = cg.make_tx([dict(frames=a(f"frames{q}"), off=a(f"off{q}"), len=a(f"len{q}"), status=a(f"txst{q}"),
                              cap_bytes=cap_bytes, cap_frames=cap_frames) for q in range(nl)], copy_bytes=64)
        rw = cg.make_fwd_rw([a(f"rwst{q}") for q in range(nl)], [a(f"port{q}") for q in range(nl)])
        seal = [cg.make_aead_burst(a(f"frames{q}"), a(f"tags{q}"), a(f"aest{q}"), cap_frames, cap_bytes, off=a(f"off{q}"),
                                   len=a(f"len{q}"), count=a(f"txst{q}"), seq_base=1000 * q, aad_bytes=34)
                for q in range(nl)]
        return batch, chk, filtered, tx, rw, seal

    batch, chk, filtered, tx, rw, seal = descs(lambda k: dev[k].addr, d_pk.addr)
    ctx.submit([batch])
    ctx.fwd_check(ng, cfg, [batch], [chk])
    ctx.tx_gather([filtered], [tx])
    ctx.fwd_rewrite(ng, cfg, [filtered], [tx], [rw])
    ctx.aead_seal(key, seal)
    ctx.sync()
    got = {k: dev[k].download(np.uint8, shapes[k]) for k in shapes}
    assert np.array_equal(got["res"].view(cg.RESULT_DT), rec)
    c = ctx.counters()
    assert all(c[k] == v for k, v in cnt.items()), (c, cnt)              # the pipeline's counters, and nothing added
    # the host mirrors chained over the device's own records and lists
    for k in ("res", "idx", "cnt"):
        host[k][:] = got[k]
    batch, chk, filtered, tx, rw, seal = descs(lambda k: host[k].ctypes.data, h_pk.ctypes.data)
    assert cg.fwd_check_host(table, cfg, [batch], [chk], nl, form == "seg") == 0
    assert cg.tx_gather_host([filtered], [tx], nl, form == "seg") == 0
    assert cg.fwd_rewrite_host(table, cfg, [filtered], [tx], [rw], nl, form == "seg") == 0
    assert cg.aead_seal_host(key, seal) == 0
    for k in shapes:
        bad = np.nonzero(got[k] != host[k])[0]
        assert bad.size == 0, (k, bad[:8], got[k][bad[:8]], host[k][bad[:8]])
    cst = host["cst"].view(np.uint32).reshape(-1, 4)
    rwst = np.stack([host[f"rwst{q}"].view(np.uint32) for q in range(nl)])
    assert cst[:, 0].sum() > 0 and cst[:, 2].sum() > 0 and cst[:, 3].sum() > 0, cst
    assert rwst[:, 0].sum() > 0 and rwst[:, 2].sum() == 0 and cst[:, 0].sum() == rwst[:, :2].sum(), (cst, rwst)
    assert np.array_equal(table_on_device(ctx, ng), table)


# ---- 7. beside a poll-mode kernel -------------------------------------------------------------------------------
def test_beside_the_poll_mode_kernel(gpu_ctx_factory, monkeypatch):
    monkeypatch.delenv("COP_PPT", raising=False)
    B, NSLOT = 1024, 4
    ctx = pipeline_ctx(gpu_ctx_factory, "dense", max_batch=B)
    table = fc.make_table(0x200, seed=1)                                 # ROUTE_NH[1] lies past its end: NO_NEIGH
    table["flags"][vp.ROUTE_NH[0]] |= 1
    cfg = cg.fwd_config(VERIFY, 5)
    slots = [l3_frames(B, m) for m in ("alt_wave", "bern_63_64")]
    dp, dr, df, dc = ctx.alloc(NSLOT * B * 64), ctx.alloc(NSLOT * B * 8), ctx.alloc(NSLOT * B * 4), ctx.alloc(64)
    for s, b in enumerate(slots):
        dp.upload(b[0], s * B * 64)
    for d in (dr, df, dc):
        d.fill(0xAB)
    ring = cg.make_ring(dp, NSLOT, B, dr, B * 64, stride=64, fwd_idx=df, fwd_count=dc)
    pk, rec, _, fwd, _ = slots[1]
    # the outputs go to mapped host memory: read below without any call that could wait for the GPU
    shapes = {"oidx": 4 * B, "ocnt": 64, "cst": 64, "frames": 64 * B, "txst": 64, "port": 4 * B, "rwst": 64}
    at, size = {}, 0
    for k, v in shapes.items():
        at[k], size = size, size + v
    hptr, dptr = ctypes.c_void_p(), ctypes.c_void_p()
    assert cg.lib().cop_host_alloc_mapped(ctx.handle, size, ctypes.byref(hptr), ctypes.byref(dptr)) == 0
    hout = np.frombuffer((ctypes.c_uint8 * size).from_address(hptr.value), dtype=np.uint8)
    hout[:] = tc.GUARD
    host = {k: tc.aligned(v, tc.GUARD) for k, v in shapes.items()}
    h_pk, h_res = tc.aligned(B * 64), tc.aligned(B * 8)
    h_pk[:], h_res[:] = pk, rec.view(np.uint8)
    h_idx, h_cnt = tc.aligned(4 * B, tc.GUARD).view(np.uint32), np.array([fwd.sum()], dtype=np.uint32)
    h_idx[:fwd.sum()] = vp.dense_list(fwd)

    def descs(a, pkts, res, idx, cnt):
        batch = cg.make_batch(pkts, B, res, 64, fwd_idx=idx, fwd_count=cnt)
        chk = cg.make_fwd_check(a("oidx"), a("ocnt"), a("cst"))
        filtered = cg.make_batch(pkts, B, res, 64, fwd_idx=a("oidx"), fwd_count=a("ocnt"))
        tx = cg.make_tx(dict(frames=a("frames"), off=None, len=None, status=a("txst"), cap_bytes=64 * B, cap_frames=B),
                        copy_bytes=64)
        return batch, chk, filtered, tx, cg.make_fwd_rw(a("rwst"), a("port"))

    try:
        with ctx.pmd_start(ring) as pm:
            pm.post(2)
            pm.wait()
            i0 = pm.info()
            assert i0["state"] == 0 and i0["completed"] == 2, i0         # running
            ng = ctx.neigh(len(table))                                   # pauses and relaunches the kernel
            ng.set(0, table)                                             # and so does the copy
            i1 = pm.info()
            batch, chk, filtered, tx, rw = descs(lambda k: dptr.value + at[k], dp.addr + B * 64, dr.addr + B * 8,
                                                 df.addr + B * 4, dc.addr + 4)
            ctx.fwd_check(ng, cfg, [batch], [chk])
            after_check = hout.copy()                                    # valid on return
            i2 = pm.info()
            ctx.tx_gather([filtered], [tx])
            ctx.fwd_rewrite(ng, cfg, [filtered], [tx], [rw])
            got = hout.copy()
            i3 = pm.info()
            pm.post(1)
            pm.wait()
            i4 = pm.info()
        batch, chk, filtered, tx, rw = descs(lambda k: host[k].ctypes.data, h_pk.ctypes.data, h_res.ctypes.data,
                                             h_idx.ctypes.data, h_cnt.ctypes.data)
        assert cg.fwd_check_host(table, cfg, [batch], [chk]) == 0
        for k in ("oidx", "ocnt", "cst"):
            assert np.array_equal(after_check[at[k]:at[k] + shapes[k]], host[k]), k
        assert cg.tx_gather_host([filtered], [tx]) == 0
        assert cg.fwd_rewrite_host(table, cfg, [filtered], [tx], [rw]) == 0
        for k in shapes:
            assert np.array_equal(got[at[k]:at[k] + shapes[k]], host[k]), k
        assert host["rwst"].view(np.uint32)[0] > 0 and 0 < host["cst"].view(np.uint32)[0] < fwd.sum()
        # create, set | check | gather, rewrite: each paused and relaunched the kernel once
        assert [i["launches"] - i0["launches"] for i in (i1, i2, i3, i4)] == [2, 3, 5, 5], (i0, i1, i2, i3, i4)
        assert i4["state"] == 0 and i4["completed"] == 3, i4
    finally:
        del hout
        cg.lib().cop_host_free_pinned(ctx.handle, hptr)


# ---- 8. errors -------------------------------------------------------------------------------------------------
def test_errors_leave_the_device_image_and_the_table_alone(gpu_ctx_factory):
    n = 300
    ctx = ctx_of(gpu_ctx_factory, "dense", max_batch=4096, max_batches=2)
    other = ctx_of(gpu_ctx_factory, "dense")
    table = fc.make_table(64, seed=1)
    ng, theirs = neigh_of(ctx, table), neigh_of(other, table)
    foreign = cg.Neigh.__new__(cg.Neigh)                                 # the other context's table, passed to this one
    foreign.ctx, foreign.handle, foreign.n_entries = ctx, theirs.handle, theirs.n_entries
    dtab, _ = ng.device_ptr()
    fresh = lambda layout="s128", m=n: fc.FwdCase(m, layout, "dense", vp.patterns(m, 256)["alt_wave"], seed=1,
                                                  table=table).with_tx()

    def refused(cases, mut=None, which="both", use=None, on=None, cfg=None):
        on, use = on or ctx, use or ng
        p = sc.Pack(on, cases)
        bs, ds, ts, rs = fc.pack_descs(p)
        if mut:
            mut(bs[0], ds[0], ts[0], rs[0])
        cf = cfg or cases[0].cfg()
        for w, call in (("check", lambda: on.fwd_check(use, cf, bs, ds)),
                        ("rewrite", lambda: on.fwd_rewrite(use, cf, bs, ts, rs))):
            if which in ("both", w):
                with pytest.raises(cg.CopError) as e:
                    call()
                assert e.value.code == EINVAL, (e.value, w)
        on.sync()
        p.check()                                                        # the whole image as it was
        assert np.array_equal(table_on_device(ctx, ng), table)

    def setf(which, field, value, q=None):
        def mut(b, d, t, r):
            obj = {"b": b, "d": d, "t": t, "r": r}[which]
            if which == "t" and q is not None:
                obj = obj.out[q]
            if which == "r":
                arr = getattr(obj, field)
                arr[0] = value(arr[0], b, d, t, r) if callable(value) else value
                return
            setattr(obj, field, value(getattr(obj, field), b, d, t, r) if callable(value) else value)
        return mut

    refused([fresh(), fresh(), fresh()])                                 # nb > max_batches
    refused([fresh(m=4097)])                                             # n > max_batch
    refused([fresh()], use=foreign)                                      # a table of another context
    refused([fresh()], cfg=cg.fwd_config(2, 0))                          # unknown flags
    for m in (setf("b", "pkts", None), setf("b", "fwd_idx", None), setf("b", "fwd_count", None),
              setf("b", "pkts", lambda v, *a: v + 8), setf("b", "data_off", 8), setf("b", "stride", 120),
              setf("b", "stride", 16), setf("b", "stride", 32), setf("b", "results", lambda v, *a: v + 4)):
        refused([fresh()], m)
    for m in (setf("d", "out_idx", None), setf("d", "out_count", None), setf("d", "status", None),
              setf("d", "status", lambda v, *a: v + 4), setf("d", "exc_idx", None), setf("d", "exc_count", None),
              setf("d", "lens", lambda v, b, *a: b.fwd_idx), setf("d", "out_idx", lambda v, b, *a: b.fwd_idx),
              setf("d", "out_count", lambda v, b, *a: b.fwd_count), setf("d", "status", lambda v, b, *a: b.pkts + 64),
              setf("d", "exc_count", lambda v, b, *a: b.results + 8), setf("d", "exc_idx", lambda v, b, d, *a: d.out_idx),
              setf("d", "status", dtab + 16)):
        refused([fresh()], m, "check")
    refused([fresh("imix")], setf("d", "lens", None), "check")
    for m in (setf("t", "copy_bytes", 32), setf("t", "slot_bytes", 100), setf("t", "frames", None, 0),
              setf("t", "status", lambda v, *a: v + 4, 0), setf("t", "cap_bytes", 1 << 32, 0),
              setf("r", "status", None), setf("r", "status", lambda v, *a: v + 4),
              setf("r", "status", lambda v, b, d, t, r: t.out[0].status),
              setf("r", "port", lambda v, b, d, t, r: t.out[0].frames + 64),
              setf("r", "port", lambda v, b, *a: b.results), setf("r", "status", dtab)):
        refused([fresh()], m, "rewrite")
    for m in (setf("t", "off", None, 0), setf("t", "len", None, 0), setf("t", "lens", None)):
        refused([fresh("imix")], m, "rewrite")
    nc = gpu_ctx_factory(stages=S, flags=cg.CFG_NO_COMPACT)
    refused([fresh()], use=neigh_of(nc, table), on=nc)
    with pytest.raises(cg.CopError) as e:
        foreign.destroy()
    assert e.value.code == EINVAL
    with pytest.raises(cg.CopError) as e:
        foreign.set(0, table[:1])
    assert e.value.code == EINVAL
    # nothing to do: 0, nothing launched
    ctx.fwd_check(ng, fresh().cfg(), [], [])
    ctx.fwd_rewrite(ng, fresh().cfg(), [], [], [])
    ctx.sync()
    # a destroyed table is no table of the context; cop_destroy frees the ones that are left
    h = ng.handle
    ng.destroy()
    assert cg.lib().cop_neigh_device_ptr(ctx.handle, h, ctypes.byref(ctypes.c_void_p()), ctypes.byref(ctypes.c_uint32())) == EINVAL
    ctx.neigh(1 << 10)
