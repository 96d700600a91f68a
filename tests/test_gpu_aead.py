"""GPU: cop_aead_seal / cop_aead_open / cop_poly1305_bulk (csrc/cop_aead.hip),
ChaCha20-Poly1305 over the frames of tx bursts on the device.

All arrays of a call sit in one device buffer whose whole image is compared
afterwards with what the host mirror (csrc/aead.c) makes of the same arrays:
the 0xAB guards round every output extent, the gaps between frames, skipped
frames, tags and ok words at and past the frame count, the padding between
the arrays and every input word must be as they were. test_aead_host.py holds
the mirror against the numpy restatement and against OpenSSL; the golden file
carries OpenSSL's own outputs to a machine without it.
"""
import ctypes

import numpy as np
import pytest

import aead_cases as ac
import copgpu as cg
import test_aead_host as th
import test_gpu_tx_gather as tg

pytestmark = pytest.mark.gpu

EINVAL = -22
PAD = ac.PAD
MATRIX = ac.matrix()
GROUPS = ("lens@", "slot:text", "slot:n", "offlen:n", "count:", "skipped", "slot:cap_cut", "seq_base")


class Pack:
    """All arrays of some bursts in one device buffer, 256 bytes apart or more."""

    def __init__(self, ctx, bursts, extra=None):
        self.bursts, self.at, pos = bursts, {}, 256
        for bi, b in enumerate(bursts):
            for name, a in b.arr.items():
                self.at[(bi, name)] = (pos, a)
                pos = (pos + a.nbytes + 511) & ~255
        for name, a in (extra or {}).items():
            self.at[(-1, name)] = (pos, a)
            pos = (pos + a.nbytes + 511) & ~255
        self.img = np.full(pos, 0x5A, dtype=np.uint8)
        for (o, a) in self.at.values():
            self.img[o:o + a.nbytes] = a.view(np.uint8)
        self.buf = ctx.alloc(pos)
        self.buf.upload(self.img)

    def addr(self, bi, name):
        return self.buf.addr + self.at[(bi, name)][0]

    def descs(self, mode):
        return [b.desc(lambda name, bi=bi: self.addr(bi, name), mode) for bi, b in enumerate(self.bursts)]

    def mirror(self, mode, key=None):
        """The image the host mirror makes of the bursts' arrays as they are in self.img."""
        hosts = []
        for bi, b in enumerate(self.bursts):
            h = ac.Burst.__new__(ac.Burst)
            h.__dict__.update(b.__dict__)
            h.arr = {name: self.img[self.at[(bi, name)][0]:][:a.nbytes].view(a.dtype).copy() for name, a in b.arr.items()}
            hosts.append(ac.aligned(h))
        assert ac.run_host(hosts, mode, key) == 0
        want = self.img.copy()
        for bi, h in enumerate(hosts):
            for name, a in h.arr.items():
                o = self.at[(bi, name)][0]
                want[o:o + a.nbytes] = a.view(np.uint8)
        return want

    def check(self, want, what=""):
        """The device image against `want`; it becomes the new self.img."""
        raw = self.buf.download(np.uint8, self.buf.nbytes)
        bad = np.nonzero(raw != want)[0]
        if bad.size:
            where = [(k, int(bad[0]) - o) for k, (o, a) in self.at.items() if o <= bad[0] < o + a.nbytes]
            raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[:8]} = {where} "
                                 f"(got {raw[bad[:8]]}, want {want[bad[:8]]})")
        self.img = raw


def seal_open(ctx, bursts, key=None, what="", restate=False):
    """Seal, compare, open, compare; the frames come back. restate: the sealed arrays against the
    numpy restatement too."""
    key_c = key or bursts[0].cg_key()
    p = Pack(ctx, bursts)
    plain = p.img.copy()
    want = p.mirror("seal", key_c)
    ctx.aead_seal(key_c, p.descs("seal"))
    ctx.sync()
    p.check(want, what + " seal")
    if restate:
        for bi, b in enumerate(bursts):
            for name, a in b.expect("seal").items():
                o = p.at[(bi, name)][0]
                assert np.array_equal(p.img[o:o + a.nbytes], a.view(np.uint8)), (what, name)
    want = p.mirror("open", key_c)
    ctx.aead_open(key_c, p.descs("open"))
    ctx.sync()
    p.check(want, what + " open")
    for bi, b in enumerate(bursts):
        o, a = p.at[(bi, "frames")]
        assert np.array_equal(p.img[o:o + a.nbytes], plain[o:o + a.nbytes]), what
    return p


# ---- 1. parity over the case matrix ---------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_matrix(gpu_ctx_factory, group):
    ctx = gpu_ctx_factory(stages=tg.S)
    names = [n for n, _ in MATRIX if n.startswith(group)]
    assert names
    for name in names:
        b = dict(ac.matrix())[name]
        seal_open(ctx, [b], what=name, restate=group in ("lens@", "skipped", "seq_base"))


def test_golden_vectors(gpu_ctx_factory):
    """OpenSSL's recorded outputs: every frame sealed on the device, one call per key."""
    ctx = gpu_ctx_factory(stages=tg.S)
    g = th.golden()
    for i in range(len(g["len"])):
        l, s = int(g["len"][i]), int(g["start"][i])
        b = ac.Burst(1, int(g["aad"][i]), lens=[l], seq_base=int(g["seq"][i]), key=g["key"][i].tobytes(),
                     salt=g["salt"][i].tobytes())
        b.arr["frames"][PAD:PAD + l] = g["plain"][s:s + l]
        p = Pack(ctx, [b])
        ctx.aead_seal(b.cg_key(), p.descs("seal"))
        ctx.sync()
        raw = p.buf.download(np.uint8, p.buf.nbytes)
        fo, to = p.at[(0, "frames")][0] + PAD, p.at[(0, "tags")][0] + PAD
        assert np.array_equal(raw[fo:fo + l], g["sealed"][s:s + l]), i
        assert np.array_equal(raw[to:to + 16], g["tag"][i]), i


def poly_burst(msgs):
    b = ac.Burst(len(msgs), 0, lens=[len(m) for m in msgs], seed=5)
    for (k, o, l), m in zip(b.walk(), msgs):
        b.arr["frames"][PAD + o:PAD + o + l] = np.frombuffer(m, np.uint8)
    return b


def test_poly1305_bulk_on_the_edge_keys(gpu_ctx_factory):
    ctx = gpu_ctx_factory(stages=tg.S)
    g = th.golden()
    msgs = [g["msg"][int(s):int(s) + int(n)].tobytes() for s, n in zip(g["mstart"], g["mlen"])]
    assert [m for _, _, m in ac.poly_edges()] == msgs           # the golden file is of these cases
    b = poly_burst(msgs)
    otk = np.ascontiguousarray(g["otk"])
    p = Pack(ctx, [b], extra={"otk": otk.reshape(-1)})
    want = p.img.copy()
    e = b.expect_poly(otk)
    for name, a in e.items():
        o = p.at[(0, name)][0]
        want[o:o + a.nbytes] = a.view(np.uint8)
    ctx.poly1305_bulk(p.descs("seal")[0], p.addr(-1, "otk"))
    ctx.sync()
    p.check(want, "poly1305_bulk")
    to = p.at[(0, "tags")][0] + PAD
    assert np.array_equal(p.img[to:to + 16 * len(msgs)].reshape(-1, 16), g["ptag"])     # OpenSSL's tags
    # long messages, every tail length, a skipped frame and a count
    rng = np.random.default_rng(8)
    lens = list(range(1, 50)) + [255, 256, 257, 2047, 2048]
    b = ac.Burst(len(lens), 0, lens=lens, seed=6, bad={7: "misaligned"}, count=len(lens) - 2)
    otk = rng.integers(0, 256, (len(lens), 32), dtype=np.uint8)
    p = Pack(ctx, [b], extra={"otk": otk.reshape(-1)})
    want = p.img.copy()
    for name, a in b.expect_poly(otk).items():
        o = p.at[(0, name)][0]
        want[o:o + a.nbytes] = a.view(np.uint8)
    ctx.poly1305_bulk(p.descs("seal")[0], p.addr(-1, "otk"))
    ctx.sync()
    p.check(want, "poly1305_bulk 2")


# ---- 2. layouts and bursts ---------------------------------------------------------------------------------
def test_several_bursts_of_different_forms_in_one_call(gpu_ctx_factory):
    ctx = gpu_ctx_factory(stages=tg.S)
    key = bytes(range(32))
    bs = [ac.Burst(65, 34, frame_bytes=64, slot_bytes=64, seed=1, key=key, seq_base=0),
          ac.Burst(0, 34, frame_bytes=64, slot_bytes=64, seed=2, key=key),
          ac.Burst(300, 14, lens=ac.imix_lens(300), seed=3, key=key, seq_base=65, count=290),
          ac.Burst(7, 0, frame_bytes=1518, slot_bytes=1520, seed=4, key=key, seq_base=1 << 33),
          ac.Burst(33, 64, frame_bytes=17, slot_bytes=32, seed=5, key=key),            # aad >= l: no keystream
          ac.Burst(40, 16, frame_bytes=2048, slot_bytes=2048, seed=6, key=key, cap_cut=2048)]
    seal_open(ctx, bs, what="six bursts")
    # more bursts than one launch carries
    many = [ac.Burst(3 + i, 12 + i, lens=ac.imix_lens(3 + i, i), seed=20 + i, key=key, seq_base=100 * i) if i % 2 else
            ac.Burst(3 + i, 34, frame_bytes=60 + i, slot_bytes=96, seed=20 + i, key=key, seq_base=100 * i)
            for i in range(20)]
    seal_open(ctx, many, what="twenty bursts")


# ---- 3. ordering ----------------------------------------------------------------------------------------------
def test_two_calls_on_two_lanes_without_sync(gpu_ctx_factory):
    ctx = gpu_ctx_factory(stages=tg.S, n_streams=2)
    b = ac.Burst(4096, 34, lens=ac.imix_lens(4096, 11), seed=31)
    p = Pack(ctx, [b])
    key = b.cg_key()
    sealed = p.mirror("seal", key)
    ctx.aead_seal(key, p.descs("seal"))       # lane 0
    ctx.aead_open(key, p.descs("open"))       # lane 1, behind lane 0
    ctx.sync()                                # once, at the end
    p.img = sealed
    p.check(p.mirror("open", key), "seal then open")
    o, a = p.at[(0, "frames")]
    assert np.array_equal(p.img[o:o + a.nbytes], b.arr["frames"])


def test_submit_tx_then_seal_then_open(gpu_ctx_factory):
    ctx = tg.pipeline_ctx(gpu_ctx_factory, "dense")
    a, ra = tg.pipeline_case(1027, "dense", "bern_63_64")
    p = tg.Pack(ctx, [a], fill_lists=True)
    bs, ts = p.descs()
    rbufs = tg.with_records(ctx, p, bs)
    o = ts[0].out[0]
    cap_frames = int(o.cap_frames)
    tags, ok, st = ctx.alloc(16 * cap_frames + 2 * PAD), ctx.alloc(4 * cap_frames + 2 * PAD), ctx.alloc(16 + 2 * PAD)
    for d in (tags, ok, st):
        d.fill(0xAB)
    key = cg.aead_key(bytes(range(1, 33)), b"\x09\0\0\0")
    burst = lambda with_ok: cg.make_aead_burst(o.frames, tags.addr + PAD, st.addr + PAD, cap_frames, int(o.cap_bytes),
                                               off=o.off, len=o.len, count=o.status,
                                               ok=ok.addr + PAD if with_ok else None, seq_base=5, aad_bytes=34)
    ctx.submit_tx(bs, ts)
    ctx.aead_seal(key, [burst(False)])
    ctx.sync()                                # one sync for the three
    # the expectation: tx_cases' restatement of the gather, then the host seal of it
    e = {k: v.copy() for k, v in a.expect[0].items()}
    W = int(e["status"][PAD // 4])
    assert 0 < W < cap_frames
    htags = np.full(16 * cap_frames + 2 * PAD, 0xAB, dtype=np.uint8)
    hst = np.full(4 + 2 * PAD // 4, 0xABABABAB, dtype=np.uint32)
    hb = cg.make_aead_burst(e["frames"].ctypes.data + PAD, htags.ctypes.data + PAD, hst.ctypes.data + PAD, cap_frames,
                            int(o.cap_bytes), off=e["off"].ctypes.data + PAD, len=e["len"].ctypes.data + PAD,
                            count=e["status"].ctypes.data + PAD, seq_base=5, aad_bytes=34)
    gathered = e["frames"].copy()
    assert cg.aead_seal_host(key, [hb]) == 0
    p.download()
    assert np.array_equal(p.got(0, "out", 0, "frames"), e["frames"])
    assert not np.array_equal(e["frames"], gathered)
    for k in ("off", "len", "status"):
        assert np.array_equal(p.got(0, "out", 0, k), e[k]), k
    assert np.array_equal(tags.download(np.uint8, tags.nbytes), htags)       # nothing at or past W, nor the guards
    assert np.array_equal(st.download(np.uint32, st.nbytes // 4), hst) and list(hst[PAD // 4:PAD // 4 + 4]) == [W, 0, 0, 0]
    tg.check_lists(p, [ra], rbufs)
    # and back
    ctx.aead_open(key, [burst(True)])
    ctx.sync()
    p.download()
    assert np.array_equal(p.got(0, "out", 0, "frames"), gathered)
    okw = ok.download(np.uint32, ok.nbytes // 4)
    assert (okw[PAD // 4:PAD // 4 + W] == 1).all() and (okw[PAD // 4 + W:] == 0xABABABAB).all()
    assert list(st.download(np.uint32, 4, PAD)) == [W, 0, 0, 0]


# ---- 4. beside a poll-mode kernel -------------------------------------------------------------------------------
def test_beside_the_poll_mode_kernel(gpu_ctx_factory, monkeypatch):
    monkeypatch.delenv("COP_PPT", raising=False)
    B, NSLOT = 1024, 4
    ctx = tg.pipeline_ctx(gpu_ctx_factory, "dense", max_batch=B)
    slots = [tg.pipeline_case(B, "dense", m) for m in ("alt_wave", "bern_63_64", "seg_tail_k", "all")]
    dp = ctx.alloc(NSLOT * B * 64)
    for s, (c, _) in enumerate(slots):
        dp.upload(c.inputs["pkts"], s * B * 64)
    dr, df, dc = ctx.alloc(NSLOT * B * 8), ctx.alloc(NSLOT * B * 4), ctx.alloc(64)
    for d in (dr, df, dc):
        d.fill(0xAB)
    ring = cg.make_ring(dp, NSLOT, B, dr, B * 64, stride=64, fwd_idx=df, fwd_count=dc)
    # the burst lives in mapped host memory: read below without any call that could wait for the GPU
    b = ac.Burst(300, 34, lens=ac.imix_lens(300, 2), seed=41, count=299, bad={17: "misaligned"})
    at, pos = {}, 0
    for name, a in b.arr.items():
        at[name] = pos
        pos = (pos + a.nbytes + 255) & ~255
    hptr, dptr = ctypes.c_void_p(), ctypes.c_void_p()
    assert cg.lib().cop_host_alloc_mapped(ctx.handle, pos, ctypes.byref(hptr), ctypes.byref(dptr)) == 0
    hout = np.frombuffer((ctypes.c_uint8 * pos).from_address(hptr.value), dtype=np.uint8)
    hout[:] = 0x5A
    for name, a in b.arr.items():
        hout[at[name]:at[name] + a.nbytes] = a.view(np.uint8)
    key = b.cg_key()

    def mirror(img, mode):
        h = ac.Burst.__new__(ac.Burst)
        h.__dict__.update(b.__dict__)
        h.arr = {name: img[at[name]:at[name] + a.nbytes].view(a.dtype).copy() for name, a in b.arr.items()}
        assert ac.run_host([ac.aligned(h)], mode, key) == 0
        want = img.copy()
        for name, a in h.arr.items():
            want[at[name]:at[name] + a.nbytes] = a.view(np.uint8)
        return want

    try:
        plain = hout.copy()
        want_sealed = mirror(plain, "seal")
        want_opened = mirror(want_sealed, "open")
        with ctx.pmd_start(ring) as pm:
            pm.post(2)
            pm.wait()
            i0 = pm.info()
            assert i0["state"] == 0 and i0["completed"] == 2, i0     # running
            ctx.aead_seal(key, [b.desc(lambda name: dptr.value + at[name], "seal")])
            got_sealed = hout.copy()                                 # valid on return
            i1 = pm.info()
            ctx.aead_open(key, [b.desc(lambda name: dptr.value + at[name], "open")])
            got_opened = hout.copy()
            pm.post(1)
            pm.wait()
            i2 = pm.info()
        assert i1["launches"] == i0["launches"] + 1 and i2["launches"] == i0["launches"] + 2, (i0, i1, i2)
        assert i2["state"] == 0 and i2["completed"] == 3, i2
        assert np.array_equal(got_sealed, want_sealed)
        assert np.array_equal(got_opened, want_opened)
        fo = at["frames"]
        assert np.array_equal(got_opened[fo:fo + b.arr["frames"].nbytes], plain[fo:fo + b.arr["frames"].nbytes])
        res = dr.download(cg.RESULT_DT, NSLOT * B)
        for s in range(3):
            assert np.array_equal(res[s * B:(s + 1) * B], slots[s][1]), f"slot {s}: records"
    finally:
        del hout
        cg.lib().cop_host_free_pinned(ctx.handle, hptr)


# ---- 5. errors ------------------------------------------------------------------------------------------------------
def test_einval_leaves_the_image_alone(gpu_ctx_factory):
    ctx = gpu_ctx_factory(stages=tg.S, max_batch=4096, max_batches=2)

    def refused(bursts, mode, mut=None, call=None):
        p = Pack(ctx, bursts)
        ds = p.descs(mode)
        if mut:
            mut(ds[0], bursts[0])
        with pytest.raises(cg.CopError) as e:
            if call:
                call(ds)
            else:
                (ctx.aead_seal if mode == "seal" else ctx.aead_open)(bursts[0].cg_key(), ds)
        assert e.value.code == EINVAL, (e.value, mode)
        ctx.sync()
        p.check(p.img.copy(), "a refused call wrote")

    slot, offlen = th.error_mutations()
    mk_slot = lambda seed=9: ac.Burst(5, 34, frame_bytes=64, slot_bytes=64, seed=seed, key=bytes(32))
    for name, mode, mut in slot:
        refused([mk_slot()], mode, mut)
    for name, mode, mut in offlen:
        refused([ac.Burst(5, 34, lens=[64, 65, 1, 2048, 16], count=5, seed=9)], mode, mut)
    refused([mk_slot(1), mk_slot(2), mk_slot(3)], "seal")                            # nb > max_batches
    refused([ac.Burst(4097, 34, frame_bytes=16, slot_bytes=16, seed=4)], "open")     # n_frames > max_batch

    # another burst's extents
    p = Pack(ctx, [mk_slot(1), mk_slot(2)])
    for field, src in (("tags", "tags"), ("status", "status"), ("frames", "frames"), ("status", "frames")):
        ds = p.descs("seal")
        setattr(ds[1], field, getattr(ds[0], src) + (64 if src == "frames" and field == "frames" else 0))
        with pytest.raises(cg.CopError) as e:
            ctx.aead_seal(cg.aead_key(bytes(32)), ds)
        assert e.value.code == EINVAL, field
    ctx.sync()
    p.check(p.img.copy(), "a refused call wrote")
    # poly1305_bulk: otk NULL, otk under tags
    b = mk_slot()
    refused([b], "seal", call=lambda ds: ctx.poly1305_bulk(ds[0], None))
    refused([b], "seal", call=lambda ds: ctx.poly1305_bulk(ds[0], ds[0].tags + 16))
    # nothing to do: 0, nothing launched, nothing needed
    ctx.aead_seal(cg.aead_key(bytes(32)), [])
    ctx.aead_open(cg.aead_key(bytes(32)), [cg.make_aead_burst(None, None, None, 0, 0)])
    ctx.sync()
