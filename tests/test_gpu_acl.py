"""GPU: cop_acl_* (csrc/cop_acl.hip), the 5-tuple ACL on the device.

The cases are acl_cases', which test_acl_host.py holds against the host mirror:
frames with random bytes everywhere but the fields set on purpose, the fixed
pattern of header kinds, every output between 0xAB guards. All arrays of a call
sit in one device buffer whose whole image is compared afterwards, so only the
outputs may differ. Expectations come from the numpy restatement (the key from
the bytes, the word by a linear scan), never from the image.
"""
import ctypes

import numpy as np
import pytest

import acl_cases as ac
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
LAYOUTS = list(ac.LAYOUTS)
PAD = ac.PAD


def ctx_of(factory, form="dense", **kw):
    return factory(stages=S, n_ports=5, flags=FLAGS[form], **kw)


def run(ctx, acl, rules, cases, counters=None, classify=True, filter=True):
    """Both calls over up to 32 cases each, one sync, the whole image compared; counters: the restatement's
    running counts, compared with the device's afterwards."""
    for lo in range(0, len(cases), 32):
        part = cases[lo:lo + 32]
        p = sc.Pack(ctx, part)
        bs, ds = p.descs()
        if classify:
            acl.classify(bs, ds)
        if filter:
            acl.filter(bs, ds)
        ctx.sync()
        for c in part:
            if classify:
                c.want_classify(rules)
            if filter:
                c.want_filter(rules, counters)
        p.check(outputs=range(len(part)))
    if counters is not None:
        got = acl.counters()
        assert np.array_equal(got, counters[:len(got)]), np.nonzero(got != counters[:len(got)])[0][:8]


def traffic_keys(seed, m=64):
    rng = np.random.default_rng(seed)
    return ac.make_keys(*(rng.integers(lo, hi, m, dtype=np.uint64) for lo, hi in
                          ((0x0A000000, 0x0B000000), (0x0A000000, 0x0B000000), (0, 1 << 16), (0, 2048), (5, 8))))


# ---- 1. both calls, every list form and size --------------------------------------------------------------
@pytest.mark.parametrize("form", list(FLAGS))
@pytest.mark.parametrize("n", sc.NS)
def test_every_list_form(gpu_ctx_factory, n, form):
    ctx = ctx_of(gpu_ctx_factory, form)
    rules = ac.traffic_rules(128)
    acl = ctx.acl(cg.AclTable(rules), cg.ACL_COUNTERS)
    keys = traffic_keys(n)
    cases = [ac.AclCase(n, LAYOUTS[(j + sc.NS.index(n)) % 4], form, fwd, KP[form], seed=j, keys=keys)
             for j, (name, fwd) in enumerate(tc.masks(n).items())]
    ctr = np.zeros(len(rules), dtype=np.uint64)
    run(ctx, acl, rules, cases, ctr)
    if n >= 255:
        st = np.sum([c.status().sum(axis=0) for c in cases], axis=0)
        assert st[0] > 0 and st[1] > 0 and st[3] > 0 and ctr.sum() > 0, st
    c = ctx.counters()
    assert c["rx"] == 0 and c["forward"] == 0, c                         # no pipeline counter is touched


# ---- 2. the row's word and lane boundaries ----------------------------------------------------------------
@pytest.mark.parametrize("n", ac.EDGE_NS)
def test_edge(gpu_ctx_factory, n):
    form = ("dense", "seg", "demux")[ac.EDGE_NS.index(n) % 3]
    ctx = ctx_of(gpu_ctx_factory, form)
    rules, keys = ac.edge(n)
    acl = ctx.acl(cg.AclTable(rules), cg.ACL_COUNTERS)
    m = 1027 if n >= 1023 else 300
    case = ac.AclCase(m, "s64", form, vp.patterns(m, 256)["bern_63_64"], KP[form], seed=n, keys=keys)
    ctr = np.zeros(max(n, 1), dtype=np.uint64)
    run(ctx, acl, rules, [case], ctr)
    st = case.status().sum(axis=0)
    if n == 0:
        assert st[1] == 0 and st[2] + st[3] == st[0] and not ctr.any()
    else:
        assert st[2] == 0 and st[1] > 0 and ctr[n // 2] > 0
        hit = {int(w) & 0xFFFFFF for w in case.words(rules) if w & ac.HIT}
        order = ac.order_of(rules)
        assert {order[r] for r in ac.EDGE_RANKS if r < n - 1} <= hit and n // 2 in hit   # the probed ranks were reached


# ---- 3. every field form, several batches and chunks, clamps ------------------------------------------------
@pytest.mark.parametrize("form", list(FLAGS))
def test_mixed_several_batches_and_clamps(gpu_ctx_factory, form):
    ctx = ctx_of(gpu_ctx_factory, form)
    rules, keys = ac.mixed()
    acl = ctx.acl(cg.AclTable(rules), cg.ACL_COUNTERS)
    K = KP[form]
    a = ac.AclCase(1027, "s64", form, vp.patterns(1027, 256)["alt_tile"], K, seed=1, keys=keys)
    b = ac.AclCase(1027, "imix", form, vp.patterns(1027, 256)["all"], K, seed=2, keys=keys[::-1])
    c = ac.AclCase(600, "s2176", form, vp.patterns(600, 256)["all"], K, seed=3, keys=keys[1000:])
    c.inputs["counts"][:] = 0xFFFFFFF0                                   # counts above what the layout holds
    junk = c.inputs["idx"] == tc.JUNK                                    # junk past the counts, now inside them
    c.inputs["idx"][junk] = 600 + 5 + np.arange(junk.sum())
    c.inputs["idx"][::7] += 600                                          # indices >= n
    # the rest of the key set, five more batches of 1027
    rest = [ac.AclCase(1027, "s128", form, None, K, seed=10 + j, keys=keys[j * 1027:]) for j in range(5)]
    ctr = np.zeros(len(rules), dtype=np.uint64)
    run(ctx, acl, rules, [a, ac.AclCase(0, "s64", form, K=K), b, c] + rest, ctr)
    st = a.status().sum(axis=0)
    assert st[0] > 0 and st[1] > 0 and st[2] > 0 and st[3] > 0, st
    # reset: read and zero
    assert np.array_equal(acl.counters(reset=True), ctr) and ctr.sum() > 0
    assert not acl.counters().any()
    assert len(acl.counters(cap=7)) == 7


# ---- 4. cop_acl_set -------------------------------------------------------------------------------------------
def test_set_1024_rules_to_1_and_back(gpu_ctx_factory):
    ctx = ctx_of(gpu_ctx_factory, "dense", n_streams=2)
    big, keys = ac.edge(1024)
    one = cg.acl_rules(1)
    one["action"] = 1
    t_big, t_one = cg.AclTable(big), cg.AclTable(one)
    acl = ctx.acl(t_one, cg.ACL_COUNTERS)                                # grows on the first set
    fwd = vp.patterns(1027, 256)["bern_63_64"]
    cases = [ac.AclCase(1027, "s64", "dense", fwd, seed=j, keys=keys) for j in range(4)]
    packs = [sc.Pack(ctx, [c]) for c in cases]
    steps = [(one, None), (big, t_big), (one, t_one), (big, t_big)]
    for (rules, table), p in zip(steps, packs):                          # no sync: set waits for what is queued
        if table is not None:
            acl.set(table)
        bs, ds = p.descs()
        acl.filter(bs, ds)
        acl.classify(bs, ds)
    ctx.sync()
    for (rules, _), c, p in zip(steps, cases, packs):
        c.want_classify(rules)
        c.want_filter(rules)
        p.check(outputs=[0])
    assert cases[0].status()[0][0] == (cases[0].skip[fwd]).sum()          # one rule that drops: only skipped ones stay
    ctr = np.zeros(1024, dtype=np.uint64)                                # set zeroed the counters: the last filter's
    cases[3].want_filter(big, ctr)
    assert np.array_equal(acl.counters(), ctr)
    acl.destroy()
    ctx.acl(t_big)


# ---- 5. the chain with no sync ---------------------------------------------------------------------------------
def pipeline_ctx(factory, form, **kw):
    ctx = factory(stages=S | F | L, n_ports=5, flags=FLAGS[form], routing_table=vp.routing_table(5), **kw)
    ctx.set_fw_table(cg.LpmTable(vp.fw_rules(), *vp.FW_CFG))
    ctx.set_route_lpm(cg.LpmTable(vp.route_rules(), 1 << 20, 1 << 16, False))
    return ctx


def l3_frames(n, mask, K=5):
    """Prescribed pipeline frames (verdict_patterns.frames) with option-less headers, no fragments, TTL 64 and
    valid checksums; ports and protocols of a few kinds."""
    fwd = vp.patterns(n, 256)[mask]
    ports = vp.port_layouts(n, 256, K)["wave"]
    pk, rec, cnt = vp.frames(vp.classes_of(mask, fwd), ports, vp.route_hit_mask(n), S | F | L)
    f = pk.reshape(n, 64)
    v4 = (f[:, 14] >> 4) == 4
    f[v4, 14] = 0x45
    f[:, 20], f[:, 21], f[:, 22] = 0, 0, 64
    f[:, 23] = np.array([6, 17, 1], dtype=np.uint8)[np.arange(n) % 3]
    f[:, 36], f[:, 37] = 0, np.array([22, 80, 53, 443, 25], dtype=np.uint16)[np.arange(n) % 5] & 0xFF
    hc = fc.csum_full(f[:, :34])
    f[:, 24], f[:, 25] = hc >> 8, hc & 0xFF
    return pk, rec, cnt, fwd, ports


def chain_rules(pk, n, fwd):
    """Rules over what the frames carry: TCP to port 22 is dropped unless it comes from the first forwarded
    packet's /16, a third of the forwarded sources are dropped by /32 rules, everything else is permitted."""
    _, k = ac.keys_of(pk, np.arange(n, dtype=np.int64) * 64)
    who = np.nonzero(fwd)[0]
    r = cg.acl_rules(3 + len(who[::3][:100]))
    r["src_ip"][0], r["src_depth"][0], r["priority"][0] = k["src"][who[0]], 16, 9
    r["proto"][1], r["proto_mask"][1], r["dport_lo"][1], r["dport_hi"][1], r["priority"][1], r["action"][1] = 6, 0xFF, 22, 22, 5, 1
    r["src_ip"][3:], r["src_depth"][3:], r["priority"][3:], r["action"][3:] = k["src"][who[::3][:100]], 32, 3, 1
    r["priority"][2] = -1
    return r


@pytest.mark.parametrize("form", list(FLAGS))
def test_submit_filter_check_gather_without_sync(gpu_ctx_factory, form):
    ctx = pipeline_ctx(gpu_ctx_factory, form, n_streams=2)
    n, K = 1027, KP[form]
    nl, cw = (K if form == "demux" else 1), max(vp.nseg(n), K)
    pk, rec, cnt, fwd, ports = l3_frames(n, "bern_63_64")
    rules = chain_rules(pk, n, fwd)
    table = cg.AclTable(rules)
    acl = ctx.acl(table, cg.ACL_COUNTERS)
    neigh = fc.make_table(1 << 20, seed=1)
    neigh["flags"][vp.ROUTE_NH[0]] |= 1
    neigh["flags"][vp.ROUTE_NH[1]] |= 1
    ng = ctx.neigh(len(neigh))
    ng.set(0, neigh)
    cfg = cg.fwd_config(cg.FWD_VERIFY_CSUM, 5)
    cap_frames, cap_bytes = n, n * 64
    shapes = {"res": n * 8, "idx": n * 4 * nl, "cnt": 4 * cw, "aidx": n * 4 * nl, "acnt": 4 * cw, "ast": 16 * nl,
              "oidx": n * 4 * nl, "ocnt": 4 * cw, "cst": 16 * nl}
    per = {"frames": cap_bytes, "off": 4 * cap_frames, "len": 4 * cap_frames, "txst": 16}
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
        flt = cg.make_acl_desc(None, a("aidx"), a("acnt"), a("ast"))
        permitted = cg.make_batch(pkts, n, a("res"), 64, fwd_idx=a("aidx"), fwd_count=a("acnt"))
        chk = cg.make_fwd_check(a("oidx"), a("ocnt"), a("cst"))
        checked = cg.make_batch(pkts, n, a("res"), 64, fwd_idx=a("oidx"), fwd_count=a("ocnt"))
        tx = cg.make_tx([dict(frames=a(f"frames{q}"), off=a(f"off{q}"), len=a(f"len{q}"), status=a(f"txst{q}"),
                              cap_bytes=cap_bytes, cap_frames=cap_frames) for q in range(nl)], copy_bytes=64)
        return batch, flt, permitted, chk, checked, tx

    batch, flt, permitted, chk, checked, tx = descs(lambda k: dev[k].addr, d_pk.addr)
    ctx.submit([batch])
    acl.filter([batch], [flt])
    ctx.fwd_check(ng, cfg, [permitted], [chk])
    ctx.tx_gather([checked], [tx])
    ctx.sync()
    got = {k: dev[k].download(np.uint8, shapes[k]) for k in shapes}
    assert np.array_equal(got["res"].view(cg.RESULT_DT), rec)
    c = ctx.counters()
    assert all(c[k] == v for k, v in cnt.items()), (c, cnt)              # the pipeline's counters, and nothing added
    # the host mirrors chained over the device's own records and lists
    for k in ("res", "idx", "cnt"):
        host[k][:] = got[k]
    batch, flt, permitted, chk, checked, tx = descs(lambda k: host[k].ctypes.data, h_pk.ctypes.data)
    ctr = np.zeros(len(rules), dtype=np.uint64)
    assert cg.acl_filter_host(table, ctr, [batch], [flt], nl, form == "seg") == 0
    assert cg.fwd_check_host(neigh, cfg, [permitted], [chk], nl, form == "seg") == 0
    assert cg.tx_gather_host([checked], [tx], nl, form == "seg") == 0
    for k in shapes:
        bad = np.nonzero(got[k] != host[k])[0]
        assert bad.size == 0, (k, bad[:8], got[k][bad[:8]], host[k][bad[:8]])
    assert np.array_equal(acl.counters(), ctr)
    # ... and the restatement agrees with the mirror on what was removed
    _, keys = ac.keys_of(pk, np.arange(n, dtype=np.int64) * 64)
    skip, _ = ac.keys_of(pk, np.arange(n, dtype=np.int64) * 64)
    w = np.where(skip, ac.SKIP, ac.scan(rules, keys))
    ast = host["ast"].view(np.uint32).reshape(-1, 4)
    assert ast[:, 0].sum() == (fwd & ((w & ac.DROP) == 0)).sum() and ast[:, 1].sum() == (fwd & ((w & ac.DROP) != 0)).sum()
    assert ast[:, 1].sum() > 0 and ctr[0] > 0 and ctr[1] > 0 and ctr[3:].sum() > 0, (ast, ctr[:4])
    txst = np.stack([host[f"txst{q}"].view(np.uint32) for q in range(nl)])
    assert 0 < txst[:, 0].sum() <= ast[:, 0].sum()


# ---- 6. beside a poll-mode kernel ------------------------------------------------------------------------------
def test_beside_the_poll_mode_kernel(gpu_ctx_factory, monkeypatch):
    monkeypatch.delenv("COP_PPT", raising=False)
    B, NSLOT = 1024, 4
    ctx = pipeline_ctx(gpu_ctx_factory, "dense", max_batch=B)
    slots = [l3_frames(B, m) for m in ("alt_wave", "bern_63_64")]
    dp, dr, df, dc = ctx.alloc(NSLOT * B * 64), ctx.alloc(NSLOT * B * 8), ctx.alloc(NSLOT * B * 4), ctx.alloc(64)
    for s, b in enumerate(slots):
        dp.upload(b[0], s * B * 64)
    for d in (dr, df, dc):
        d.fill(0xAB)
    ring = cg.make_ring(dp, NSLOT, B, dr, B * 64, stride=64, fwd_idx=df, fwd_count=dc)
    pk, rec, _, fwd, _ = slots[1]
    rules = chain_rules(pk, B, fwd)
    table = cg.AclTable(rules)
    # the outputs go to mapped host memory: read below without any call that could wait for the GPU
    shapes = {"words": 4 * B, "oidx": 4 * B, "ocnt": 64, "st": 64}
    at, size = {}, 0
    for k, v in shapes.items():
        at[k], size = size, size + v
    hptr, dptr = ctypes.c_void_p(), ctypes.c_void_p()
    assert cg.lib().cop_host_alloc_mapped(ctx.handle, size, ctypes.byref(hptr), ctypes.byref(dptr)) == 0
    hout = np.frombuffer((ctypes.c_uint8 * size).from_address(hptr.value), dtype=np.uint8)
    hout[:] = tc.GUARD
    host = {k: tc.aligned(v, tc.GUARD) for k, v in shapes.items()}
    h_pk = tc.aligned(B * 64)
    h_pk[:] = pk
    h_idx, h_cnt = tc.aligned(4 * B, tc.GUARD).view(np.uint32), np.array([fwd.sum()], dtype=np.uint32)
    h_idx[:fwd.sum()] = vp.dense_list(fwd)

    def descs(a, pkts, idx, cnt):
        return (cg.make_batch(pkts, B, None, 64, fwd_idx=idx, fwd_count=cnt),
                cg.make_acl_desc(a("words"), a("oidx"), a("ocnt"), a("st")))

    try:
        with ctx.pmd_start(ring) as pm:
            pm.post(2)
            pm.wait()
            i0 = pm.info()
            assert i0["state"] == 0 and i0["completed"] == 2, i0         # running
            acl = ctx.acl(table, cg.ACL_COUNTERS)                        # pauses and relaunches the kernel
            i1 = pm.info()
            batch, d = descs(lambda k: dptr.value + at[k], dp.addr + B * 64, df.addr + B * 4, dc.addr + 4)
            acl.classify([batch], [d])
            after_classify = hout.copy()                                 # valid on return
            i2 = pm.info()
            acl.filter([batch], [d])
            got = hout.copy()
            i3 = pm.info()
            ctr = acl.counters()
            acl.set(table)
            zeroed = acl.counters()
            i4 = pm.info()
            acl.destroy()                                                # a counted ACL: both frees inside the pause
            i5 = pm.info()
            pm.post(1)
            pm.wait()
            i6 = pm.info()
        batch, d = descs(lambda k: host[k].ctypes.data, h_pk.ctypes.data, h_idx.ctypes.data, h_cnt.ctypes.data)
        want_ctr = np.zeros(len(rules), dtype=np.uint64)
        assert cg.acl_classify_host(table, [batch], [d]) == 0
        assert np.array_equal(after_classify[at["words"]:at["words"] + 4 * B], host["words"])
        assert (after_classify[at["oidx"]:] == tc.GUARD).all()           # classify wrote the words and nothing else
        assert cg.acl_filter_host(table, want_ctr, [batch], [d]) == 0
        for k in shapes:
            assert np.array_equal(got[at[k]:at[k] + shapes[k]], host[k]), k
        st = host["st"].view(np.uint32)
        assert st[0] > 0 and st[1] > 0 and st[0] + st[1] == fwd.sum(), st[:4]
        assert np.array_equal(ctr, want_ctr) and not zeroed.any()
        # create | classify | filter | read, set, read | destroy | nothing: each paused and relaunched the kernel once
        assert [i["launches"] - i0["launches"] for i in (i1, i2, i3, i4, i5, i6)] == [1, 2, 3, 6, 7, 7], (i0, i1, i2, i3, i4, i5, i6)
        assert i6["state"] == 0 and i6["completed"] == 3, i6
    finally:
        del hout
        cg.lib().cop_host_free_pinned(ctx.handle, hptr)


# ---- 7. errors -------------------------------------------------------------------------------------------------
def image_words(ctx, acl, rules, keys):
    """The ACL still classifies as its rules say: the image (and the layout the runtime keeps) is untouched."""
    c = ac.AclCase(300, "s64", "dense", seed=77, keys=keys)
    run(ctx, acl, rules, [c], filter=False)


def test_errors_leave_the_device_image_and_the_counters_alone(gpu_ctx_factory):
    n = 300
    ctx = ctx_of(gpu_ctx_factory, "dense", max_batch=4096, max_batches=2)
    other = ctx_of(gpu_ctx_factory, "dense")
    rules = ac.traffic_rules(128)
    table, keys = cg.AclTable(rules), traffic_keys(5)
    acl, theirs = ctx.acl(table, cg.ACL_COUNTERS), other.acl(table, cg.ACL_COUNTERS)
    foreign = cg.Acl.__new__(cg.Acl)                                     # the other context's ACL, passed to this one
    foreign.ctx, foreign.handle, foreign.flags, foreign.n_rules = ctx, theirs.handle, theirs.flags, theirs.n_rules
    seeded = ac.AclCase(n, "s64", "dense", seed=3, keys=keys)            # counters that are not zero
    ctr = np.zeros(len(rules), dtype=np.uint64)
    run(ctx, acl, rules, [seeded], ctr, classify=False)
    assert ctr.sum() > 0
    fresh = lambda layout="s128", m=n: ac.AclCase(m, layout, "dense", vp.patterns(m, 256)["alt_wave"], seed=1, keys=keys)

    def refused(cases, mut=None, which="both", use=None, on=None):
        on, use = on or ctx, use or acl
        p = sc.Pack(on, cases)
        bs, ds = p.descs()
        if mut:
            mut(bs[0], ds[0])
        for w, call in (("classify", lambda: use.classify(bs, ds)), ("filter", lambda: use.filter(bs, ds))):
            if which in ("both", w):
                with pytest.raises(cg.CopError) as e:
                    call()
                assert e.value.code == EINVAL, (e.value, w)
        on.sync()
        p.check()                                                        # the whole image as it was

    def setf(which, field, value):
        def mut(b, d):
            obj = {"b": b, "d": d}[which]
            setattr(obj, field, value(getattr(obj, field), b, d) if callable(value) else value)
        return mut

    refused([fresh(), fresh(), fresh()])                                 # nb > max_batches
    refused([fresh(m=4097)])                                             # n > max_batch
    refused([fresh()], use=foreign)                                      # an ACL of another context
    for m in (setf("b", "pkts", None), setf("b", "pkts", lambda v, *a: v + 8), setf("b", "data_off", 8),
              setf("b", "stride", 120), setf("b", "stride", 12), setf("b", "stride", 16), setf("b", "stride", 32)):
        refused([fresh()], m)
    for m in (setf("d", "words", None), setf("d", "words", lambda v, *a: v + 2),
              setf("d", "words", lambda v, b, d: b.pkts + 64)):
        refused([fresh()], m, "classify")
    refused([fresh("imix")], setf("d", "words", lambda v, b, d: b.offsets), "classify")
    for m in (setf("b", "fwd_idx", None), setf("b", "fwd_count", None), setf("d", "out_idx", None),
              setf("d", "out_count", None), setf("d", "status", None), setf("d", "status", lambda v, *a: v + 4),
              setf("d", "out_idx", lambda v, b, d: b.fwd_idx), setf("d", "out_count", lambda v, b, d: b.fwd_count),
              setf("d", "status", lambda v, b, d: b.pkts + 64), setf("d", "out_count", lambda v, b, d: d.out_idx + 16)):
        refused([fresh()], m, "filter")
    # an output over the ACL's image or its counters
    img, img_bytes, dctr, nr = acl.device_ptr()
    assert img and dctr and nr == len(rules) and img_bytes == table.report.image_bytes
    for at in (img + 64, img + img_bytes - 16, dctr, dctr + 8 * nr - 16):
        refused([fresh()], setf("d", "status", at), "filter")
        refused([fresh()], setf("d", "out_count", at), "filter")
        refused([fresh()], setf("d", "words", at), "classify")
    nc = gpu_ctx_factory(stages=S, flags=cg.CFG_NO_COMPACT)
    refused([fresh()], which="filter", use=nc.acl(table), on=nc)
    for bad in (lambda: foreign.destroy(), lambda: foreign.set(table), lambda: foreign.counters(),
                lambda: ctx.acl(table).counters(), lambda: ctx.acl(table, 2)):
        with pytest.raises(cg.CopError) as e:
            bad()
        assert e.value.code == EINVAL
    # nothing to do: 0, nothing launched
    acl.classify([], [])
    acl.filter([], [])
    ctx.sync()
    assert np.array_equal(acl.counters(), ctr)                           # no refused call counted
    image_words(ctx, acl, rules, keys)
    # a destroyed ACL is no ACL of the context; cop_destroy frees the ones that are left
    h = acl.handle
    acl.destroy()
    assert cg.lib().cop_acl_counters_read(ctx.handle, h, None, 0, 0) == EINVAL
    ctx.acl(table, cg.ACL_COUNTERS)
