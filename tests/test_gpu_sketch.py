"""GPU: cop_sketch_* (csrc/cop_sketch.hip), per-source packet accounting and
policing on the device.

The cases are sketch_cases', which test_sketch_host.py holds against the host
mirror: frames with random bytes everywhere but the fields set on purpose,
police outputs between 0xAB guards. All arrays of a call sit in one device
buffer whose whole image is compared afterwards, so only outputs may differ;
the counters come back through cop_sketch_read and are compared word for word
with the numpy restatement (sketch_cases.Spec).
"""
import ctypes
import itertools

import numpy as np
import pytest

import copgpu as cg
import sketch_cases as sc
import tx_cases as tc
import verdict_patterns as vp

pytestmark = pytest.mark.gpu

S, F = vp.S, vp.F
EINVAL, ENOSPC = -22, -28
FLAGS = {"dense": 0, "seg": cg.CFG_SEG_LISTS, "demux": cg.CFG_DEMUX_PORTS}
KP = {"dense": 1, "seg": 1, "demux": 5}
FWD = 1 << cg.FORWARD


def ctx_of(factory, form="dense", **kw):
    return factory(stages=S, n_ports=5, flags=FLAGS[form], **kw)


def sketch_of(ctx, spec):
    return cg.Sketch(ctx, spec.cfg())


def preload(ctx, sk, counters):
    dptr, words = sk.device_ptr()
    assert words == counters.size
    a = np.ascontiguousarray(counters)
    assert cg.lib().cop_memcpy_h2d(ctx.handle, ctypes.c_void_p(dptr), a.ctypes.data, a.nbytes) == 0


def same(got, want):
    assert got.shape == want.shape
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, (bad[0][:6], bad[1][:6], got[bad][:6], want[bad][:6], int(got.sum()), int(want.sum()))


# ---- 1. update -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.NS)
def test_update_every_layout_and_kind(gpu_ctx_factory, n):
    ctx = ctx_of(gpu_ctx_factory)
    specs = [sc.Spec(r, lc, k, kd, seed=n + 3) for (r, lc), (k, kd) in
             zip(((1, 4), (4, 10), (4, 4), (1, 20)), ((0, 32), (1, 24), (0, 8), (1, 1)))]
    sks, want = [sketch_of(ctx, s) for s in specs], [s.zeros() for s in specs]
    cases = [sc.SkCase(n, kind, layout, seed=j) for j, (layout, kind) in enumerate(itertools.product(sc.LAYOUTS, sc.KINDS))]
    p = sc.Pack(ctx, cases)
    bs, _ = p.descs()
    for j, c in enumerate(cases):
        x, mask = (j + n) % len(specs), sc.VERDICT_MASKS[j % len(sc.VERDICT_MASKS)]
        sks[x].update([bs[j]], mask)                  # no sync between them
        c.update(specs[x], want[x], mask)
    ctx.sync()
    p.check()                                          # nothing but the counters was written
    for x in range(len(specs)):
        same(sks[x].read(), want[x])
    c = ctx.counters()
    assert c["rx"] == 0 and c["forward"] == 0, c       # no pipeline counter is touched


@pytest.mark.parametrize("log2_cols", [4, 10, 20])
@pytest.mark.parametrize("rows", [1, 4])
def test_update_every_config(gpu_ctx_factory, rows, log2_cols):
    ctx = ctx_of(gpu_ctx_factory)
    cases = [sc.SkCase(1027, kind, "s64", seed=3) for kind in ("heavy4", "same24")]
    p = sc.Pack(ctx, cases)
    bs, _ = p.descs(with_results=False)                # verdict_mask 0: results may be NULL
    for key, key_depth in itertools.product((0, 1), (32, 24, 8, 1)):
        spec = sc.Spec(rows, log2_cols, key, key_depth, seed=0xC0FFEE)
        sk = sketch_of(ctx, spec)
        sk.update(bs, 0)
        want = spec.zeros()
        for c in cases:
            c.update(spec, want)
        same(sk.read(), want)
        sk.destroy()
    p.check()


def test_three_layouts_in_one_call_and_two_updates_without_sync(gpu_ctx_factory):
    ctx = ctx_of(gpu_ctx_factory, n_streams=2)
    spec = sc.Spec(4, 10, seed=11)
    sk = sketch_of(ctx, spec)
    cases = [sc.SkCase(1027, "heavy4", "s2176", seed=1), sc.SkCase(0, "one", "s64"), sc.SkCase(600, "mixed", "imix", seed=2),
             sc.SkCase(257, "same24", "rec16", seed=3), sc.SkCase(vp.LONG_N, "heavy4", "s64", seed=4)]
    p = sc.Pack(ctx, cases)
    bs, _ = p.descs()
    want = spec.zeros()
    sk.update(bs[:4], 1)                               # lane 0
    sk.update(bs[4:], 0)                               # lane 1, behind lane 0
    sk.update(bs[2:3], 4)
    ctx.sync()
    for c in cases[:4]:
        c.update(spec, want, 1)
    cases[4].update(spec, want, 0)
    cases[2].update(spec, want, 4)
    p.check()
    same(sk.read(), want)


def test_counters_carry_into_the_high_word(gpu_ctx_factory):
    ctx = ctx_of(gpu_ctx_factory)
    spec = sc.Spec(4, 10, seed=13)
    sk = sketch_of(ctx, spec)
    case = sc.SkCase(8, "one", "s64")
    pre = spec.zeros()
    pre[np.arange(4), spec.col(case.keys(spec)[:1])[:, 0].astype(np.int64)] = (1 << 32) - 3
    preload(ctx, sk, pre)
    p = sc.Pack(ctx, [case])
    sk.update(p.descs()[0], 0)
    want = pre.copy()
    case.update(spec, want)
    got = sk.read()
    same(got, want)
    assert int(spec.est(got, case.keys(spec)[:1])[0]) == (1 << 32) + 5


# ---- 2. behind the pipeline --------------------------------------------------------------------------
def pipeline_ctx(factory, form, **kw):
    ctx = factory(stages=S | F, n_ports=5, flags=FLAGS[form], routing_table=vp.routing_table(5), **kw)
    ctx.set_fw_table(cg.LpmTable(vp.fw_rules(), *vp.FW_CFG))
    return ctx


class PipelineBatch:
    """Prescribed frames (verdict_patterns.frames) with device arrays the pipeline is to fill."""

    def __init__(self, ctx, n, form, mask, K=5):
        self.n, self.form = n, form
        self.fwd = vp.patterns(n, 256)[mask]
        self.ports = vp.port_layouts(n, 256, K)["wave"]
        self.pk, self.rec, _ = vp.frames(vp.classes_of(mask, self.fwd), self.ports)
        self.ipv4, self.src, self.dst = sc.fields(self.pk, np.arange(n, dtype=np.int64) * 64, False)
        self.d_pk = ctx.alloc(n * 64)
        self.d_pk.upload(self.pk)
        nl = K if form == "demux" else 1
        self.d_res, self.d_idx, self.d_cnt = ctx.alloc(n * 8), ctx.alloc(n * 4 * nl), ctx.alloc(4 * max(vp.nseg(n), nl))
        for d in (self.d_res, self.d_idx, self.d_cnt):
            d.fill(0xAB)
        self.batch = cg.make_batch(self.d_pk, n, self.d_res, 64, fwd_idx=self.d_idx, fwd_count=self.d_cnt)

    def counting(self, mask):
        return self.ipv4 & (((mask >> self.rec["verdict"].astype(np.int64)) & 1).astype(bool) if mask else True)


def test_submit_then_update_of_the_forwarded_without_sync(gpu_ctx_factory):
    ctx = pipeline_ctx(gpu_ctx_factory, "dense", n_streams=2)
    spec = sc.Spec(4, 14, seed=17)
    sk = sketch_of(ctx, spec)
    b = PipelineBatch(ctx, vp.LONG_N, "dense", "alt_tile")
    ctx.submit([b.batch])                              # lane 0
    sk.update([b.batch], FWD)                          # lane 1: behind lane 0, or it reads 0xAB records
    ctx.sync()
    assert np.array_equal(b.d_res.download(cg.RESULT_DT, b.n), b.rec)
    want = spec.zeros()
    spec.add(want, spec.key_of(b.src)[b.counting(FWD)])
    assert 0 < b.counting(FWD).sum() < b.n
    same(sk.read(), want)


# ---- 3. query, decay --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1027])
def test_query(gpu_ctx_factory, n):
    ctx = ctx_of(gpu_ctx_factory)
    for spec in (sc.Spec(4, 10, 0, 32, seed=1), sc.Spec(1, 4, 1, 24, seed=2), sc.Spec(4, 20, 0, 8, seed=3)):
        sk = sketch_of(ctx, spec)
        case = sc.SkCase(1027, "heavy4", "s64", seed=4)
        addr = (case.dst if spec.key else case.src)[:n]
        ips = np.concatenate([addr[: n // 2], addr[: n - n // 2] ^ np.uint64(0x01000001)]).astype(np.uint32)
        out = np.full(n + 16, sc.U64_MAX - 5, dtype=np.uint64)
        p = sc.Pack(ctx, [case], {"ips": np.concatenate([ips, np.zeros(1, np.uint32)]), "out": out})
        sk.update(p.descs()[0], 0)
        sk.query(p.x("ips"), n, p.x("out") + 64)       # no sync in between
        ctx.sync()
        ctr = spec.zeros()
        case.update(spec, ctr)
        want = out.copy()
        want[8:8 + n] = spec.est(ctr, spec.key_of(ips))
        p.check(extra_want={"out": want})
        same(sk.read(), ctr)
        sk.destroy()


@pytest.mark.parametrize("shift", [1, 7, 63, 64])
def test_decay(gpu_ctx_factory, shift):
    ctx = ctx_of(gpu_ctx_factory)
    for spec in (sc.Spec(1, 4, seed=1), sc.Spec(4, 10, seed=2), sc.Spec(3, 17, seed=3)):
        sk = sketch_of(ctx, spec)
        same(sk.read(), spec.zeros())                  # zero at creation
        pre = np.random.default_rng(shift).integers(0, 1 << 64, (spec.rows, spec.cols), dtype=np.uint64)
        for j, v in enumerate((sc.U64_MAX, 1 << 63, (1 << shift) - 1 if shift < 64 else sc.U64_MAX)):
            pre[0, j] = np.uint64(v)
        preload(ctx, sk, pre)
        sk.decay(shift)
        ctx.sync()
        same(sk.read(), pre >> np.uint64(shift) if shift < 64 else spec.zeros())


# ---- 4. police ------------------------------------------------------------------------------------------
def police(ctx, sk, spec, ctr, cases):
    for lo in range(0, len(cases), 32):
        part = cases[lo:lo + 32]
        p = sc.Pack(ctx, part)
        bs, ps = p.descs()
        sk.police(bs, ps)
        ctx.sync()
        for c in part:
            c.police(spec, ctr)
        p.check(outputs=range(len(part)))              # the batch, its lists and its records are not written
    same(sk.read(), ctr)                               # ... nor the sketch


def trained(ctx, spec, n):
    """A sketch that has seen the heavy4 traffic twice; (sketch, its counters)."""
    sk = sketch_of(ctx, spec)
    traffic = sc.SkCase(max(n, 64), "heavy4", "s64", seed=8)
    p = sc.Pack(ctx, [traffic])
    bs, _ = p.descs()
    sk.update(bs + bs, 0)
    ctr = spec.zeros()
    traffic.update(spec, ctr)
    traffic.update(spec, ctr)
    return sk, ctr


@pytest.mark.parametrize("form", list(FLAGS))
@pytest.mark.parametrize("n", sc.NS)
def test_police_every_list_form(gpu_ctx_factory, n, form):
    ctx = ctx_of(gpu_ctx_factory, form)
    spec = sc.Spec(4, 10, n % 2, 32 if n % 3 else 24, seed=n)
    sk, ctr = trained(ctx, spec, n)
    layouts, kinds = list(sc.LAYOUTS), ("heavy4", "mixed", "same24", "one", "distinct")
    cases = []
    for j, (name, fwd) in enumerate(tc.masks(n).items()):
        c0 = sc.SkCase(n, kinds[j % 5], layouts[j % 5], form, fwd, KP[form], seed=8)
        for th in (0, 1, c0.median_threshold(spec, ctr), sc.U64_MAX):
            c = sc.SkCase(n, kinds[j % 5], layouts[j % 5], form, fwd, KP[form], seed=8, threshold=th)
            cases.append(c)
    police(ctx, sk, spec, ctr, cases)


@pytest.mark.parametrize("form", list(FLAGS))
def test_police_many_chunks_and_clamps(gpu_ctx_factory, form):
    ctx = ctx_of(gpu_ctx_factory, form)
    n, K = vp.LONG_N, KP[form]
    spec = sc.Spec(4, 10, seed=21)
    sk, ctr = trained(ctx, spec, 1027)
    a = sc.SkCase(n, "heavy4", "s64", form, vp.patterns(n, 256)["alt_tile"], K, seed=8)
    a.threshold = 100      # between the light keys' estimates and the heavy ones'
    b = sc.SkCase(n, "mixed", "rec16", form, vp.patterns(n, 256)["all"], K, seed=8, threshold=3)
    # the clamps: counts above what the layout holds, indices >= n
    c = sc.SkCase(600, "heavy4", "s64", form, vp.patterns(600, 256)["all"], K, seed=8)
    c.inputs["counts"][:] = 0xFFFFFFF0
    junk = c.inputs["idx"] == tc.JUNK
    c.inputs["idx"][junk] = 600 + 5 + np.arange(junk.sum())
    c.inputs["idx"][::7] += 600
    c.threshold = c.median_threshold(spec, ctr)
    police(ctx, sk, spec, ctr, [a, sc.SkCase(0, "one", "s64", form, K=K), b, c])
    kept = int(a.expect[0]["status"][tc.PAD // 4])
    assert 0 < kept < int(a.inputs["counts"].sum())


@pytest.mark.parametrize("form", ["dense", "seg", "demux"])
def test_pipeline_update_police_tx_gather_without_sync(gpu_ctx_factory, form):
    """cop_submit, cop_sketch_update(FORWARD), cop_sketch_police, cop_tx_gather of the police's lists, one sync."""
    ctx = pipeline_ctx(gpu_ctx_factory, form, n_streams=2)
    n, K = 1027, KP[form]
    spec = sc.Spec(4, 12, cg.SKETCH_KEY_SRC, 16, seed=23)   # per /16: the three accept rules' /16s are the heavy keys
    sk = sketch_of(ctx, spec)
    b = PipelineBatch(ctx, n, form, "bern_63_64")
    key = spec.key_of(b.src)
    ctr = spec.zeros()
    spec.add(ctr, key[b.counting(FWD)])
    est = spec.est(ctr, key)
    th = 50
    kept = b.fwd & (~b.ipv4 | (est < np.uint64(th)))
    assert 0 < kept.sum() < b.fwd.sum()
    # the tx case of the filtered list: its bursts and what they must hold
    t = tc.slot_case(n, form, kept, 64, 0, 64, ports=b.ports, K=K, pk=b.pk)
    d_oidx, d_ocnt, d_st = ctx.alloc(n * 4 * (K if form == "demux" else 1)), ctx.alloc(4 * max(vp.nseg(n), K)), ctx.alloc(16 * K)
    for d in (d_oidx, d_ocnt, d_st):
        d.fill(0xAB)
    bursts = {}
    for q, o in enumerate(t.outs):
        for k, a in o.items():
            bursts[(q, k)] = ctx.alloc(a.nbytes)
            bursts[(q, k)].upload(a)
    filtered, tx = t.descs({"pkts": b.d_pk.addr, "idx": d_oidx.addr, "counts": d_ocnt.addr}.get,
                           lambda q, k: bursts[(q, k)].addr)
    ctx.submit([b.batch])
    sk.update([b.batch], FWD)
    sk.police([b.batch], [cg.make_police(th, d_oidx, d_ocnt, d_st)])
    ctx.tx_gather([filtered], [tx])
    ctx.sync()
    same(sk.read(), ctr)
    t.check(lambda q, k: bursts[(q, k)].download(t.outs[q][k].dtype, t.outs[q][k].size))
    st = d_st.download(np.uint32, 4 * K)
    assert int(st[0::4][:1 if form != "demux" else K].sum()) == int(kept.sum())
    assert int(st[1::4][:1 if form != "demux" else K].sum()) == int(b.fwd.sum() - kept.sum())


# ---- 5. beside a poll-mode kernel ------------------------------------------------------------------------
def test_beside_the_poll_mode_kernel(gpu_ctx_factory, monkeypatch):
    monkeypatch.delenv("COP_PPT", raising=False)
    B, NSLOT = 1024, 4
    ctx = pipeline_ctx(gpu_ctx_factory, "dense", max_batch=B)
    spec = sc.Spec(4, 10, cg.SKETCH_KEY_SRC, 16, seed=29)
    slots = [PipelineBatch(ctx, B, "dense", m) for m in ("alt_wave", "bern_63_64")]
    dp, dr, df, dc = ctx.alloc(NSLOT * B * 64), ctx.alloc(NSLOT * B * 8), ctx.alloc(NSLOT * B * 4), ctx.alloc(64)
    for s, b in enumerate(slots):
        dp.upload(b.pk, s * B * 64)
    for d in (dr, df, dc):
        d.fill(0xAB)
    ring = cg.make_ring(dp, NSLOT, B, dr, B * 64, stride=64, fwd_idx=df, fwd_count=dc)
    b1 = slots[1]
    batch = cg.make_batch(dp.addr + B * 64, B, dr.addr + B * 8, 64, fwd_idx=df.addr + B * 4, fwd_count=dc.addr + 4)
    d_ips = ctx.alloc(4 * B)
    d_ips.upload(b1.src.astype(np.uint32))
    # the outputs go to mapped host memory: read below without any call that could wait for the GPU
    at = {"est": 0, "out_idx": 8 * B, "out_count": 8 * B + 4 * B, "status": 8 * B + 4 * B + 64}
    size = at["status"] + 64
    hptr, dptr = ctypes.c_void_p(), ctypes.c_void_p()
    assert cg.lib().cop_host_alloc_mapped(ctx.handle, size, ctypes.byref(hptr), ctypes.byref(dptr)) == 0
    hout = np.frombuffer((ctypes.c_uint8 * size).from_address(hptr.value), dtype=np.uint8)
    hout[:] = tc.GUARD
    try:
        with ctx.pmd_start(ring) as pm:
            pm.post(2)
            pm.wait()
            i0 = pm.info()
            assert i0["state"] == 0 and i0["completed"] == 2, i0     # running
            sk = sketch_of(ctx, spec)
            sk.update([batch], FWD)
            ctr = sk.read()                                          # valid on return
            want = spec.zeros()
            spec.add(want, spec.key_of(b1.src)[b1.counting(FWD)])
            same(ctr, want)
            i1 = pm.info()
            sk.query(d_ips, B, dptr.value + at["est"])
            est = hout[:8 * B].view(np.uint64).copy()                # valid on return
            i2 = pm.info()
            th = 50
            sk.police([batch], [cg.make_police(th, dptr.value + at["out_idx"], dptr.value + at["out_count"],
                                               dptr.value + at["status"])])
            got = hout.copy()
            i3 = pm.info()
            sk.decay(1)
            same(sk.read(), want >> np.uint64(1))
            pm.post(1)
            pm.wait()
            i4 = pm.info()
        assert np.array_equal(est, spec.est(want, spec.key_of(b1.src)))
        kept = vp.dense_list(b1.fwd & (~b1.ipv4 | (est < np.uint64(th))))
        assert 0 < len(kept) < b1.fwd.sum()
        assert got[at["out_count"]:at["out_count"] + 4].view(np.uint32)[0] == len(kept)
        assert np.array_equal(got[at["out_idx"]:at["out_idx"] + 4 * len(kept)].view(np.uint32), kept)
        assert (got[at["out_idx"] + 4 * len(kept):at["out_idx"] + 4 * B] == tc.GUARD).all()
        assert got[at["status"]:at["status"] + 16].view(np.uint32).tolist() == [len(kept), int(b1.fwd.sum()) - len(kept), 0, 0]
        # create, update, read | query | police | decay, read: each paused and relaunched the kernel once
        assert [i["launches"] - i0["launches"] for i in (i1, i2, i3, i4)] == [3, 4, 5, 7], (i0, i1, i2, i3, i4)
        assert i4["state"] == 0 and i4["completed"] == 3, i4
    finally:
        del hout
        cg.lib().cop_host_free_pinned(ctx.handle, hptr)


# ---- 6. errors ----------------------------------------------------------------------------------------------
def test_errors_leave_the_device_image_and_the_counters_alone(gpu_ctx_factory):
    n = 300
    fwd = vp.patterns(n, 256)["alt_wave"]
    ctx = ctx_of(gpu_ctx_factory, "dense", max_batch=4096, max_batches=2)
    other = ctx_of(gpu_ctx_factory, "dense")
    spec = sc.Spec(4, 10, seed=2)
    sk, theirs = sketch_of(ctx, spec), sketch_of(other, spec)
    foreign = cg.Sketch.__new__(cg.Sketch)              # the other context's sketch, passed to this one
    foreign.ctx, foreign.cfg, foreign.handle, foreign.words = ctx, theirs.cfg, theirs.handle, theirs.words
    pre = np.full((4, 1 << 10), 7, dtype=np.uint64)
    preload(ctx, sk, pre)
    dctr, _ = sk.device_ptr()
    fresh = lambda m=n, layout="s128": sc.SkCase(m, "heavy4", layout, "dense", vp.patterns(m, 256)["alt_wave"], seed=1, threshold=5)

    def refused(call, cases, mut=None, code=EINVAL, use=None, on=None):
        on, use = on or ctx, use or sk
        p = sc.Pack(on, cases, {"ips": np.zeros(8, np.uint32), "out": np.full(8, 9, np.uint64)})
        bs, ps = p.descs()
        if mut:
            mut(bs[0], ps[0], p)
        with pytest.raises(cg.CopError) as e:
            call(use, bs, ps, p)
        assert e.value.code == code, (e.value, mut)
        on.sync()
        p.check()                                       # the whole image as it was
        same(sk.read(), pre)

    def setf(which, field, value):
        def mut(b, p, pack):
            obj = {"b": b, "p": p}[which]
            setattr(obj, field, value(getattr(obj, field), b, p) if callable(value) else value)
        return mut

    upd = lambda s, bs, ps, p: s.update(bs, 1)
    pol = lambda s, bs, ps, p: s.police(bs, ps)
    for call in (upd, pol):
        refused(call, [fresh(), fresh(), fresh()])                               # nb > max_batches
        refused(call, [fresh(4097)])                                             # n > max_batch
        refused(call, [fresh()], use=foreign)                                    # a sketch of another context
        for m in (setf("b", "pkts", None), setf("b", "pkts", lambda v, b, p: v + 8), setf("b", "data_off", 8),
                  setf("b", "stride", 12), setf("b", "stride", 120)):
            refused(call, [fresh()], m)
    refused(upd, [fresh()], setf("b", "results", None))                          # verdict_mask != 0
    refused(lambda s, bs, ps, p: s.update(bs, 1 << 5), [fresh()])
    for m in (setf("b", "fwd_idx", None), setf("b", "fwd_count", None), setf("p", "out_idx", None),
              setf("p", "out_count", None), setf("p", "status", None), setf("p", "status", lambda v, b, p: v + 4),
              setf("p", "out_idx", lambda v, b, p: b.fwd_idx), setf("p", "out_idx", lambda v, b, p: b.fwd_idx + 4 * (n - 1)),
              setf("p", "out_count", lambda v, b, p: b.fwd_count), setf("p", "status", lambda v, b, p: b.pkts + 64),
              setf("p", "out_count", lambda v, b, p: b.results + 8), setf("p", "status", lambda v, b, p: dctr + 16)):
        refused(pol, [fresh()], m)
    nc = gpu_ctx_factory(stages=S, flags=cg.CFG_NO_COMPACT)
    refused(pol, [fresh()], use=sketch_of(nc, spec), on=nc)
    for shift in (0, 65):
        refused(lambda s, bs, ps, p: s.decay(shift), [fresh()])
    refused(lambda s, bs, ps, p: s.decay(1), [fresh()], use=foreign)
    refused(lambda s, bs, ps, p: s.query(p.x("ips"), 8, p.x("out")), [fresh()], use=foreign)
    for a, o in ((None, 0), (0, None), (0, 4), (2, 0)):
        refused(lambda s, bs, ps, p: s.query(None if a is None else p.x("ips") + a, 4, None if o is None else p.x("out") + o),
                [fresh()])
    refused(lambda s, bs, ps, p: s.query(p.x("out") + 8, 4, p.x("out")), [fresh()])      # out over ips
    refused(lambda s, bs, ps, p: s.query(p.x("ips"), 4, dctr + 64), [fresh()])          # out over the counters
    refused(lambda s, bs, ps, p: s.read(cap_words=4095), [fresh()], code=ENOSPC)
    for kw in (dict(rows=0), dict(rows=5), dict(log2_cols=3), dict(log2_cols=25), dict(key=2), dict(key_depth=0),
               dict(key_depth=33)):
        with pytest.raises(cg.CopError) as e:
            ctx.sketch(**kw)
        assert e.value.code == EINVAL, kw
    with pytest.raises(cg.CopError) as e:
        foreign.destroy()
    assert e.value.code == EINVAL
    # nothing to do: 0, nothing launched
    sk.update([], 1)
    sk.police([], [])
    sk.query(None, 0, None)
    ctx.sync()
    same(sk.read(), pre)
    # a destroyed sketch is no sketch of the context; cop_destroy frees the ones that are left
    h = sk.handle
    sk.destroy()
    assert cg.lib().cop_sketch_decay(ctx.handle, h, 1) == EINVAL
    ctx.sketch(4, 20)
