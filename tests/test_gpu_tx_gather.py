"""GPU: cop_tx_gather / cop_submit_tx (csrc/cop_tx.hip), forwarded frames
packed into tx bursts on the device.

Source frames hold random bytes, so a misplaced 16-byte piece shows. Every
output extent (frames, off, len, status) lies between 0xAB guards, and all the
arrays of a call sit in one device buffer whose whole image is compared
afterwards: the guards, the gaps between slot frames, off / len past the
written frames, the padding between the arrays and every input word (packets,
offsets, lens, lists, counts) must be as they were. Expected values come from
tx_cases.restate (numpy), which test_tx_gather_host.py holds against
cop_tx_gather_host.
"""
import ctypes

import numpy as np
import pytest

import copgpu as cg
import tx_cases as tc
import verdict_patterns as vp

pytestmark = pytest.mark.gpu

S, F = vp.S, vp.F
EINVAL, EBUSY = -22, -16
NS = (0, 1, 255, 256, 257, 768, 1027)
FLAGS = {"dense": 0, "seg": cg.CFG_SEG_LISTS, "demux": cg.CFG_DEMUX_PORTS}
# (stride, data_off) x copy_bytes where it fits x slot_bytes in {copy_bytes, copy_bytes + 48}
SLOT_SHAPES = [(st, do, cb, cb + gap) for st, do in ((64, 0), (128, 0), (2176, 128))
               for cb in (16, 48, 64, 80, 1024, 1040, 2048) if cb <= st - do for gap in (0, 48)]


class Pack:
    """All arrays of some cases in one device buffer, 256 bytes apart or more."""

    def __init__(self, ctx, cases, fill_lists=False):
        self.cases, self.at, pos = cases, {}, 256
        for ci, c in enumerate(cases):
            for name, a in c.inputs.items():
                self.at[(ci, "in", 0, name)] = (pos, a)
                pos = (pos + a.nbytes + 511) & ~255
            for q, o in enumerate(c.outs):
                for k, a in o.items():
                    self.at[(ci, "out", q, k)] = (pos, a)
                    pos = (pos + a.nbytes + 511) & ~255
        self.img = np.full(pos, 0x5A, dtype=np.uint8)
        for (ci, kind, q, name), (o, a) in self.at.items():
            self.img[o:o + a.nbytes] = a.view(np.uint8)
            if fill_lists and name in ("idx", "counts"):     # the pipeline is to write them
                self.img[o:o + a.nbytes] = tc.GUARD
        self.buf = ctx.alloc(pos)
        self.buf.upload(self.img)
        self.raw = None

    def addr(self, ci, kind, q, name):
        return self.buf.addr + self.at[(ci, kind, q, name)][0] if (ci, kind, q, name) in self.at else None

    def descs(self):
        out = [c.descs(lambda name, ci=ci: self.addr(ci, "in", 0, name), lambda q, k, ci=ci: self.addr(ci, "out", q, k))
               for ci, c in enumerate(self.cases)]
        return [b for b, _ in out], [t for _, t in out]

    def got(self, ci, kind, q, name):
        o, a = self.at[(ci, kind, q, name)]
        return self.raw[o:o + a.nbytes].view(a.dtype)

    def download(self):
        self.raw = self.buf.download(np.uint8, self.buf.nbytes)

    def check(self, whole=True):
        self.download()
        for ci, c in enumerate(self.cases):
            c.check(lambda q, k, ci=ci: self.got(ci, "out", q, k))
        if whole:   # nothing but the outputs changed
            want = self.img.copy()
            for (ci, kind, q, name), (o, a) in self.at.items():
                if kind == "out":
                    want[o:o + a.nbytes] = self.cases[ci].expect[q][name].view(np.uint8)
            bad = np.nonzero(self.raw != want)[0]
            assert bad.size == 0, f"bytes outside the outputs changed at {bad[:8]}"

    def untouched(self):
        self.download()
        bad = np.nonzero(self.raw != self.img)[0]
        assert bad.size == 0, f"a refused call wrote at {bad[:8]}"


def gather(ctx, cases):
    for lo in range(0, len(cases), 32):
        p = Pack(ctx, cases[lo:lo + 32])
        ctx.tx_gather(*p.descs())
        ctx.sync()
        p.check()


def ctx_of(factory, form, **kw):
    return factory(stages=S, n_ports=5, flags=FLAGS[form], **kw)


# ---- 1. the kernel alone, slot batches ------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "seg", "demux"])
@pytest.mark.parametrize("n", NS)
def test_slot_batches(gpu_ctx_factory, n, form):
    ctx = ctx_of(gpu_ctx_factory, form)
    K = 5 if form == "demux" else 1
    m = list(tc.masks(n).items())
    lay = vp.port_layouts(n, 256, 5) if n else {}
    cases = []
    for j in range(max(len(m), len(SLOT_SHAPES))):       # every mask and every shape at least once
        name, fwd = m[j % len(m)]
        st, do, cb, sb = SLOT_SHAPES[(j + NS.index(n)) % len(SLOT_SHAPES)]
        ports = lay[("mod", "wave", "port4")[j % 3]] if n else np.zeros(0, dtype=np.int64)
        cases.append(tc.slot_case(n, form, fwd, st, do, cb, sb, ports=ports, K=K))
    gather(ctx, cases)


# ---- 2. IMIX ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "seg"])
@pytest.mark.parametrize("n", NS)
def test_imix_batches(gpu_ctx_factory, n, form):
    ctx = ctx_of(gpu_ctx_factory, form)
    gather(ctx, [tc.imix_case(n, form, fwd, data_off=16 * (j % 2)) for j, fwd in enumerate(tc.masks(n).values())])


def test_imix_clamp_null_off_len_and_demux(gpu_ctx_factory):
    n = 1027
    p = vp.patterns(n, 256)
    ctx = ctx_of(gpu_ctx_factory, "dense")
    gather(ctx, [tc.imix_case(n, "dense", p["bern_63_64"], lens_cycle=(0, 5000, 64, 17)),
                 tc.imix_case(n, "dense", p["alt_wave"], no_off_len=True),
                 tc.slot_case(n, "dense", p["seg_tail_k"], 128, 0, 80, 128)])        # both kinds in one call
    ctx = ctx_of(gpu_ctx_factory, "demux")
    gather(ctx, [tc.imix_case(n, "demux", p[k], ports=vp.port_layouts(n, 256, 5)[l], K=5)
                 for k, l in (("all", "wave"), ("bern_1_64", "mod"), ("alt_seg", "port4"))])


# ---- 3. more than 256 chunks --------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["all", "alt_tile"])
def test_more_than_256_chunks(gpu_ctx_factory, mask):
    n = vp.LONG_N
    fwd = vp.patterns(n, 256)[mask]
    gather(ctx_of(gpu_ctx_factory, "seg"), [tc.slot_case(n, "seg", fwd, 64, 0, 64)])
    gather(ctx_of(gpu_ctx_factory, "dense"), [tc.imix_case(n, "dense", fwd, lens_cycle=(64,))])


# ---- 4. capacity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "seg"])
@pytest.mark.parametrize("src", ["slot", "slot_gap", "imix"])
def test_capacity(gpu_ctx_factory, src, form):
    n = 1027
    fwd = vp.patterns(n, 256)["bern_63_64"]

    def case_of(caps):
        if src == "imix":
            return tc.imix_case(n, form, fwd, caps=caps)
        return tc.slot_case(n, form, fwd, 128, 0, 80, 80 if src == "slot" else 128, caps=caps)

    cases = [c for _, c in tc.cap_cases(case_of)]
    for c in cases:
        st = c.expect[0]["status"][tc.PAD // 4:tc.PAD // 4 + 4]
        assert st[0] + st[2] == len(c.lists[0])
    gather(ctx_of(gpu_ctx_factory, form), cases)


# ---- 5. chained with the pipeline ---------------------------------------------------------------------
def pipeline_ctx(factory, form, **kw):
    ctx = factory(stages=S | F, n_ports=5, flags=FLAGS[form], routing_table=vp.routing_table(5), **kw)
    ctx.set_fw_table(cg.LpmTable(vp.fw_rules(), *vp.FW_CFG))
    return ctx


def pipeline_case(n, form, mask, layout="wave"):
    """(TxCase over the prescribed frames, prescribed records)."""
    fwd = vp.patterns(n, 256)[mask]
    ports = vp.port_layouts(n, 256, 5)[layout]
    pk, rec, _ = vp.frames(vp.classes_of(mask, fwd), ports)
    return tc.slot_case(n, form, fwd, 64, 0, 64, ports=ports, K=5 if form == "demux" else 1, pk=pk), rec


def with_records(ctx, pack, batches):
    """Give every batch a records array in its own buffer; returns the buffers."""
    bufs = []
    for b in batches:
        r = ctx.alloc(max(b.n, 1) * 8)
        r.fill(0xAB)
        b.results = r.addr
        bufs.append(r)
    return bufs


def check_lists(pack, recs, rbufs):
    """Records and the covered list words against the prescription."""
    for ci, c in enumerate(pack.cases):
        got = rbufs[ci].download(cg.RESULT_DT, c.n)
        assert np.array_equal(got, recs[ci]), f"batch {ci}: records"
        cnt, idx, want = pack.got(ci, "in", 0, "counts"), pack.got(ci, "in", 0, "idx"), c.inputs["idx"]
        assert np.array_equal(cnt, c.inputs["counts"]), (ci, cnt[:8], c.inputs["counts"][:8])
        covered = want != tc.JUNK
        assert np.array_equal(idx[covered], want[covered]), f"batch {ci}: lists"


@pytest.mark.parametrize("form", ["dense", "seg", "demux"])
def test_submit_tx_two_batches(gpu_ctx_factory, form):
    ctx = pipeline_ctx(gpu_ctx_factory, form)
    (a, ra), (b, rb) = pipeline_case(1027, form, "bern_63_64"), pipeline_case(600, form, "alt_wave", "mod")
    p = Pack(ctx, [a, b], fill_lists=True)
    bs, ts = p.descs()
    rbufs = with_records(ctx, p, bs)
    ctx.submit_tx(bs, ts)
    ctx.sync()
    p.check(whole=False)
    check_lists(p, [ra, rb], rbufs)
    # what cop_submit alone gives: the same records, counts and covered list words
    p2 = Pack(ctx, [a, b], fill_lists=True)
    bs2, _ = p2.descs()
    rbufs2 = with_records(ctx, p2, bs2)
    ctx.submit(bs2)
    ctx.sync()
    p2.download()
    check_lists(p2, [ra, rb], rbufs2)
    for ci in range(2):
        assert np.array_equal(rbufs[ci].download(np.uint8, p.cases[ci].n * 8),
                              rbufs2[ci].download(np.uint8, p.cases[ci].n * 8))
    # the gather touched no counter: two submits' worth
    c = ctx.counters()
    forwarded = sum(len(l) for x in (a, b) for l in x.lists)
    assert c["rx"] == 2 * (1027 + 600) and c["forward"] == 2 * forwarded, c


def test_gather_behind_submits_on_two_lanes(gpu_ctx_factory):
    ctx = pipeline_ctx(gpu_ctx_factory, "dense", n_streams=2)
    big = vp.LONG_N
    (a, ra), (b, rb) = pipeline_case(big, "dense", "alt_tile"), pipeline_case(1027, "dense", "seg_head_k")
    p = Pack(ctx, [a, b], fill_lists=True)
    bs, ts = p.descs()
    rbufs = with_records(ctx, p, bs)
    ctx.submit([bs[0]])          # lane 0
    ctx.submit([bs[1]])          # lane 1
    ctx.tx_gather(bs, ts)        # lane 0, behind lane 1 too
    ctx.sync()                   # once, at the end
    p.check(whole=False)
    check_lists(p, [ra, rb], rbufs)


# ---- 6. beside a poll-mode kernel ------------------------------------------------------------------------
def test_beside_the_poll_mode_kernel(gpu_ctx_factory, monkeypatch):
    monkeypatch.delenv("COP_PPT", raising=False)
    B, NSLOT = 1024, 4
    ctx = pipeline_ctx(gpu_ctx_factory, "dense", max_batch=B)
    slots = [pipeline_case(B, "dense", m) for m in ("alt_wave", "bern_63_64", "seg_tail_k", "all")]
    dp = ctx.alloc(NSLOT * B * 64)
    for s, (c, _) in enumerate(slots):
        dp.upload(c.inputs["pkts"], s * B * 64)
    dr, df, dc = ctx.alloc(NSLOT * B * 8), ctx.alloc(NSLOT * B * 4), ctx.alloc(64)
    for d in (dr, df, dc):
        d.fill(0xAB)
    ring = cg.make_ring(dp, NSLOT, B, dr, B * 64, stride=64, fwd_idx=df, fwd_count=dc)
    # the burst goes to mapped host memory: read below without any call that could wait for the GPU
    c1 = slots[1][0]
    o = c1.outs[0]
    at, pos = {}, 0
    for k in ("frames", "off", "len", "status"):
        at[k] = pos
        pos = (pos + o[k].nbytes + 255) & ~255
    hptr, dptr = ctypes.c_void_p(), ctypes.c_void_p()
    assert cg.lib().cop_host_alloc_mapped(ctx.handle, pos, ctypes.byref(hptr), ctypes.byref(dptr)) == 0
    hout = np.frombuffer((ctypes.c_uint8 * pos).from_address(hptr.value), dtype=np.uint8)
    hout[:] = tc.GUARD
    batch, tx = c1.descs(lambda name: None, lambda q, k: dptr.value + at[k])
    batch.pkts = dp.addr + B * 64
    batch.results, batch.fwd_idx, batch.fwd_count = dr.addr + B * 8, df.addr + B * 4, dc.addr + 4
    try:
        with ctx.pmd_start(ring) as pm:
            pm.post(2)
            pm.wait()
            i0 = pm.info()
            assert i0["state"] == 0 and i0["completed"] == 2, i0     # running
            ctx.tx_gather([batch], [tx])
            got = hout.copy()                                        # valid on return
            with pytest.raises(cg.CopError) as e:
                ctx.submit_tx([batch], [tx])
            assert e.value.code == EBUSY
            pm.post(1)
            pm.wait()
            i1 = pm.info()
        assert i1["state"] == 0 and i1["completed"] == 3 and i1["launches"] == i0["launches"] + 1, (i0, i1)
        c1.check(lambda q, k: got[at[k]:at[k] + o[k].nbytes].view(o[k].dtype))
        res = dr.download(cg.RESULT_DT, NSLOT * B)
        for s in range(3):
            assert np.array_equal(res[s * B:(s + 1) * B], slots[s][1]), f"slot {s}: records"
        assert (dr.download(np.uint8, B * 8, 3 * B * 8) == 0xAB).all()       # slot 3 was never posted
    finally:
        del hout
        cg.lib().cop_host_free_pinned(ctx.handle, hptr)


# ---- 7. errors ----------------------------------------------------------------------------------------------
def test_einval_leaves_the_outputs_alone(gpu_ctx_factory):
    n = 300
    fwd = vp.patterns(n, 256)["alt_wave"]

    def refused(ctx, cases, mut=None, code=EINVAL, call="tx_gather"):
        p = Pack(ctx, cases)
        bs, ts = p.descs()
        if mut:
            mut(bs[0], ts[0], ts[0].out[0])
        with pytest.raises(cg.CopError) as e:
            getattr(ctx, call)(bs, ts)
        assert e.value.code == code, (e.value, mut)
        ctx.sync()
        p.untouched()

    ctx = ctx_of(gpu_ctx_factory, "dense", max_batch=4096, max_batches=2)
    slot = lambda: tc.slot_case(n, "dense", fwd, 128, 0, 64, 64)
    imix = lambda: tc.imix_case(n, "dense", fwd)

    def setf(which, field, value):
        def mut(b, t, o):
            obj = {"b": b, "t": t, "o": o}[which]
            setattr(obj, field, value(getattr(obj, field), b, t) if callable(value) else value)
        return mut

    refused(ctx, [slot(), slot(), slot()])                                  # nb > max_batches
    refused(ctx, [tc.slot_case(4097, "dense", vp.patterns(4097, 256)["none"])])   # n > max_batch
    for m in (setf("b", "fwd_idx", None), setf("b", "fwd_count", None), setf("b", "stride", 12),
              setf("b", "stride", 120), setf("b", "data_off", 8), setf("t", "copy_bytes", 0), setf("t", "copy_bytes", 40),
              setf("t", "copy_bytes", 144), setf("t", "slot_bytes", 48), setf("t", "slot_bytes", 72),
              setf("t", "lens", lambda v, b, t: b.fwd_idx), setf("o", "frames", lambda v, b, t: v + 8),
              setf("o", "frames", None), setf("o", "status", lambda v, b, t: v + 4), setf("o", "status", None),
              setf("o", "cap_bytes", 1 << 32), setf("o", "frames", lambda v, b, t: b.pkts + 64),
              setf("o", "status", lambda v, b, t: b.fwd_idx), setf("o", "off", lambda v, b, t: b.fwd_count - 16)):
        refused(ctx, [slot()], m)
        refused(ctx, [slot()], m, call="submit_tx")
    for m in (setf("t", "lens", None), setf("t", "copy_bytes", 64), setf("o", "len", lambda v, b, t: t.lens)):
        refused(ctx, [imix()], m)
    big = gpu_ctx_factory(stages=S, max_batch=1 << 21)
    refused(big, [slot()], setf("b", "n", 1 << 21))                         # n * COP_TX_MAX_FRAME >= 2^32
    refused(gpu_ctx_factory(stages=S, flags=cg.CFG_NO_COMPACT), [slot()])
    # nb == 0: nothing launched, nothing needed
    ctx.tx_gather([], [])
    ctx.submit_tx([], [])
    ctx.sync()
