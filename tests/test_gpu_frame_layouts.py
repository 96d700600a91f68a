"""GPU: every header-load path on frames that name their own packet.

The loaders that bring a packet's fields into a lane's registers (csrc/
cop_device.h load_step / gather_step, load_off_imix / load_step_imix; csrc/
cop_tile.h: the 16- and 12-byte record loads and the per-lane slot loads of
tile_body, plain and system-coherent, and the windowed pipelines of
tile_steps_v) run here on identity frames (tests/frame_layouts.py; the
oracle agrees with their prescription on the host, test_frame_layouts.py):
packet g's record is a function of g, so a packet read from a wrong lane,
chunk, step, slot or lap is named in the failure. Every byte a loader moves
but must ignore is filler; every case runs with two filler seeds and must
give the prescribed records, forward list and count both times, bit for bit,
with the 0xAB guards around the records, after the list's last entry and
around the counts untouched.

One-shot launches assert the instantiation their parameters name through
Context.launch_plan() / launch_forms(), poll-mode kernels through
Pmd.info()["kernel_name"].
"""
import functools

import numpy as np
import pytest

import copgpu as cg
import frame_layouts as fl
import verdict_patterns as vp
from test_gpu_verdict_patterns import Guarded, knobs

pytestmark = pytest.mark.gpu

S, F, L = fl.S, fl.F, fl.L
DIR = cg.CFG_LPM_FORCE_DIR24
# route form -> (prefixes of the route table, context flags)
ROUTES = {"lds": (4096, 0), "dir": (4096, DIR), "trie": (fl.WINDOW, cg.CFG_LPM_TRIE), "bkt": (fl.WINDOW, cg.CFG_LPM_BKT),
          "auto": (fl.WINDOW, 0)}          # 16,384 prefixes leave LDS: DIR-24-8
FORM_OF = {"auto": "dir"}
LPM_ARG = {"lds": 1, "dir": 2, "auto": 2, "trie": 3, "bkt": 4}   # COPK_TBL_* in a kernel's name


@functools.lru_cache(maxsize=None)
def fw_table():
    return fl.fw_table()


@functools.lru_cache(maxsize=None)
def route_table(R):
    return fl.route_table(R)


def make_ctx(factory, route="auto", stages=S | F | L, flags=0):
    R, rflags = ROUTES[route]
    ctx = factory(stages=stages, n_ports=fl.K, flags=flags | rflags, routing_table=fl.routing_table())
    ctx.set_fw_table(fw_table())
    if stages & L:
        ctx.set_route_lpm(route_table(R))
        assert ctx.route_form() == FORM_OF.get(route, route)
    return ctx, R


def check_batch(name, want, rec, lst, cnt, seg=False, **whokw):
    """One batch's records, forward list, count and the guard words behind
    the list's last entry against the prescription."""
    got = rec.view(cg.RESULT_DT)
    assert np.array_equal(got, want), fl.describe(name, got, want, **whokw)
    fwd = want["verdict"] == cg.FORWARD
    lst, cnt = lst.view(np.uint32), cnt.view(np.uint32)
    if not seg:
        w = vp.dense_list(fwd)
        assert cnt[0] == len(w), f"{name}: count {cnt[0]}, prescribed {len(w)}"
        assert np.array_equal(lst[:len(w)], w), f"{name}: forward list"
        assert (lst[len(w):] == 0xABABABAB).all(), f"{name}: list words written past entry {len(w)}"
        return
    wc, wl = vp.seg_lists(fwd)
    assert np.array_equal(cnt, wc), f"{name}: segment counts {cnt[:8]}, prescribed {wc[:8]}"
    for s, w in enumerate(wl):
        seg_words = lst[s * vp.SEG:(s + 1) * vp.SEG]
        assert np.array_equal(seg_words[:len(w)], w), f"{name}: segment {s} (length {len(w)})"
        # (a segment goes out in 16-byte chunks: cop_device.h st_list_chunk)
        assert (seg_words[-(-len(w) // 4) * 4:] == 0xABABABAB).all(), f"{name}: segment {s} written past its chunk"


def submit_check(ctx, lays, stages, R, ppt, layout, route=None):
    """The layouts as the batches of one cop_submit: outputs against the
    prescription, and the instantiation that ran."""
    at, pos = [], 0
    for lay in lays:
        pos = -(-pos // 256) * 256
        o = None
        if lay.offsets is not None:
            o = -(-(pos + lay.image.nbytes) // 16) * 16
        at.append((pos, o))
        pos = (o + lay.offsets.nbytes) if o is not None else pos + lay.image.nbytes
    dp = ctx.alloc(pos + 16)
    for lay, (a, o) in zip(lays, at):
        dp.upload(lay.image, a)
        if o is not None:
            dp.upload(lay.offsets, o)
    ns = [len(lay.g) for lay in lays]
    rec = Guarded.packed(ctx, [n * 8 for n in ns])
    lst = Guarded.packed(ctx, [n * 4 for n in ns])
    cnt = Guarded.packed(ctx, [4] * len(ns), align=4)
    for x in (rec, lst, cnt):
        x.fill()
    ctx.submit([cg.make_batch(dp, n, rec.addr(b), pkts_offset=at[b][0] + lay.shift,
                              offsets=None if at[b][1] is None else dp.addr + at[b][1],
                              fwd_idx=lst.addr(b), fwd_count=cnt.addr(b), **lay.kw)
                for b, (lay, n) in enumerate(zip(lays, ns))])
    ctx.sync()
    assert ctx.launch_plan() == (layout, ppt), (ctx.launch_plan(), layout, ppt)
    if route is not None:
        assert ctx.launch_forms()[:2] == ("lds", FORM_OF.get(route, route)), ctx.launch_forms()
    r, l, k = rec.read("records"), lst.read("lists"), cnt.read("counts")
    for b, lay in enumerate(lays):
        first = fl.span_of(lay.g)
        assert first + ns[b] <= fl.WINDOW          # every batch of the submit inside one window of identities
        check_batch(f"batch {b} {lay.name} n={ns[b]} first={first} ppt={ppt}", fl.records(lay.g, stages, R),
                    r[b], l[b], k[b], lo=0, first=first, ppt=ppt, R=R, stages=stages,
                    others=[(f"batch {q}", fl.span_of(x.g), len(x.g)) for q, x in enumerate(lays) if q != b])
    for x in (dp, rec.buf, lst.buf, cnt.buf):
        x.free()


# ---------------------------------------------------------------------------
# one-shot: every loader at every tile edge

# name -> (builder(n, first, seed, R), $COP_LOADS or None, the launch's layout)
LOADERS = {
    "slots": (lambda n, f, s, R: fl.slots(n, f, s, 64, 0, R), "strided", "slots"),
    "coalesced": (lambda n, f, s, R: fl.slots(n, f, s, 64, 0, R), None, "coalesced"),
    "imix": (lambda n, f, s, R: fl.imix(n, f, s, "phases", 0, R), None, "imix"),
    "hdr16": (lambda n, f, s, R: fl.hdr16(n, f, s, R), None, "hdr16"),
    "hdr12": (lambda n, f, s, R: fl.hdr12(n, f, s, 4 * ((n + n // 64) % 4), R), None, "hdr16"),
}
EDGES = [(ld, ppt, rt) for ld in LOADERS for ppt in (1, 4, 8)
         for rt in (("lds", "dir", "trie", "bkt") if ld in ("coalesced", "imix") else ("auto",))]


def edge_sizes(T):
    return [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 65]


@pytest.mark.parametrize("loader,ppt,route", EDGES)
def test_oneshot_loaders_at_tile_edges(gpu_ctx_factory, monkeypatch, loader, ppt, route):
    """Each loader at 1, 4 and 8 packets per lane: batches that end one
    packet into, at, and one packet short of a wave, a step and a tile, as
    the unequal batches of one submit (tiles assigned by block ranges) and
    again as equal batches of T + 65 (tiles interleaved by division). The
    batches' identities are 1021 apart, so a read from a neighbour batch is
    named too."""
    build, loads, layout = LOADERS[loader]
    knobs(monkeypatch, COP_PPT=ppt, **({"COP_LOADS": loads} if loads else {}))
    ctx, R = make_ctx(gpu_ctx_factory, route)
    T = 256 * ppt
    sizes = sorted(set(edge_sizes(T)))
    for seed in fl.FILL_SEEDS:
        submit_check(ctx, [build(n, 1021 * b, seed, R) for b, n in enumerate(sizes)], S | F | L, R, ppt, layout, route)
        submit_check(ctx, [build(T + 65, 1021 * b, seed, R) for b in range(3)], S | F | L, R, ppt, layout, route)


STRIDES = (48, 64, 80, 96, 112, 128, 2176)
HEADROOMS = (0, 16, 48, 128)


@pytest.mark.parametrize("loads,layout", [("strided", "slots"), (None, "coalesced")])
@pytest.mark.parametrize("ppt", [4, 8])
def test_oneshot_strides_and_headroom(gpu_ctx_factory, monkeypatch, loads, layout, ppt):
    """Both slot loaders over every stride x data_off, 2T + 65 packets each:
    the 28 geometries as the batches of one submit."""
    knobs(monkeypatch, COP_PPT=ppt, **({"COP_LOADS": loads} if loads else {}))
    ctx, R = make_ctx(gpu_ctx_factory)
    n = 2 * 256 * ppt + 65
    for seed in fl.FILL_SEEDS:
        lays = [fl.slots(n, 431 * b, seed, st, do, R)
                for b, (st, do) in enumerate((st, do) for st in STRIDES for do in HEADROOMS)]
        assert len(lays) == 28
        submit_check(ctx, lays, S | F | L, R, ppt, layout, "auto")


@pytest.mark.parametrize("ppt", [1, 4, 8])
def test_oneshot_imix_offset_policies(gpu_ctx_factory, monkeypatch, ppt):
    """Every offset policy x data_off {0, 16}: all four 16-byte phases mod 64
    within one wave's step, descending and shuffled offsets, the minimal
    48-byte pitch, and every packet at one offset. 8 packets per lane is an
    instantiation the launch never picks for IMIX on its own (choose_ppt)."""
    knobs(monkeypatch, COP_PPT=ppt)
    ctx, R = make_ctx(gpu_ctx_factory)
    n = 2 * 256 * ppt + 65
    for seed in fl.FILL_SEEDS:
        lays = [fl.imix(n, 577 * b, seed, p, do, R)
                for b, (p, do) in enumerate((p, do) for p in fl.IMIX_POLICIES for do in (0, 16))]
        submit_check(ctx, lays, S | F | L, R, ppt, "imix", "auto")


SWEEP_LAYOUTS = {
    "slots": (lambda n, s, kw: fl.slots(n, 0, s, 64, 0, **kw), "strided", "slots"),
    "coalesced": (lambda n, s, kw: fl.slots(n, 0, s, 64, 0, **kw), None, "coalesced"),
    "imix": (lambda n, s, kw: fl.imix(n, 0, s, "phases", 0, **kw), None, "imix"),
    "hdr16": (lambda n, s, kw: fl.hdr16(n, 0, s, **kw), None, "hdr16"),
    "hdr12": (lambda n, s, kw: fl.hdr12(n, 0, s, 8, **kw), None, "hdr16"),
}


@pytest.mark.parametrize("stages", [S | F | L, F | L])
@pytest.mark.parametrize("loader", list(SWEEP_LAYOUTS))
def test_oneshot_field_sweeps(gpu_ctx_factory, monkeypatch, loader, stages):
    """All 65,536 EtherTypes and all 256 values of byte 14 (byte 15 0x00 and
    0xFF) through each layout at the launch's own tile size: one EtherType
    passes the parse stage, sixteen values of byte 14 are version 4, and
    with no parse stage nothing reads the EtherType."""
    build, loads, layout = SWEEP_LAYOUTS[loader]
    knobs(monkeypatch, **({"COP_LOADS": loads} if loads else {}))
    ctx, R = make_ctx(gpu_ctx_factory, stages=stages)
    et = np.arange(65536)
    b14, b15 = np.tile(np.arange(256), 2), np.repeat([0x00, 0xFF], 256)
    for seed in fl.FILL_SEEDS:
        for name, n, kw, want in (("ethertype", 65536, dict(et=et), fl.ethertype_records(stages)),
                                  ("version", 512, dict(b14=b14, b15=b15), fl.version_records(stages))):
            lay = build(n, seed, kw)
            dp = ctx.alloc(lay.image.nbytes + (lay.offsets.nbytes if lay.offsets is not None else 0) + 16)
            dp.upload(lay.image)
            o = None
            if lay.offsets is not None:
                o = -(-lay.image.nbytes // 16) * 16
                dp.upload(lay.offsets, o)
            rec, lst, cnt = (Guarded.packed(ctx, [sz]) for sz in (n * 8, n * 4, 4))
            for x in (rec, lst, cnt):
                x.fill()
            ctx.submit([cg.make_batch(dp, n, rec.addr(), pkts_offset=lay.shift, offsets=None if o is None else dp.addr + o,
                                      fwd_idx=lst.addr(), fwd_count=cnt.addr(), **lay.kw)])
            ctx.sync()
            assert ctx.launch_plan()[0] == layout, ctx.launch_plan()
            got = rec.read("records")[0].view(cg.RESULT_DT)
            for lo in range(0, n, fl.WINDOW):      # the identity repeats every window: name within one
                hi = min(n, lo + fl.WINDOW)
                assert np.array_equal(got[lo:hi], want[lo:hi]), fl.describe(
                    f"{name} sweep through {lay.name}, packets {lo}..", got[lo:hi], want[lo:hi], lo, lo,
                    ctx.launch_plan()[1], stages=stages)
            check_batch(f"{name} sweep through {lay.name}", want, rec.read("records")[0], lst.read("list")[0],
                        cnt.read("count")[0], lo=0, stages=stages)
            for x in (dp, rec.buf, lst.buf, cnt.buf):
                x.free()


# ---------------------------------------------------------------------------
# offsets past 4 GiB

BIG = (1 << 32) + (64 << 10)
HALF = 32 << 10
DECOY_FIRST = 8192            # identities of the frames at the buffer's start: what a wrapped address reads


def big_slab(ctx, seed, data_off):
    """One device buffer of 2^32 + 64 KiB of which only the first 64 KiB
    (decoy identity frames DECOY_FIRST + k at 64 k) and the 64 KiB around
    2^32 are written. Packets at 64-byte pitch, in shuffled order, with
    offsets[i] + data_off in [2^32 - 32 KiB, 2^32 + 32 KiB) as far as
    offsets up to 0xFFFFFFC0 reach: -> (buffer, offsets, identities)."""
    try:
        dp = ctx.alloc(BIG)
    except cg.CopError as e:
        if "out of memory" in str(e).lower():
            pytest.skip(f"no {BIG} bytes of device memory for one buffer: {e}")
        raise
    decoy = fl.slots(1024, DECOY_FIRST, seed, 64, 0)
    dp.upload(decoy.image, 0)
    start = (1 << 32) - HALF + 64 * np.arange(1024, dtype=np.int64)        # offsets[i] + data_off
    start = start[start - data_off <= 0xFFFFFFC0]
    start = start[np.random.default_rng(0x5EEDF404).permutation(len(start))]
    g = np.arange(len(start))
    window, _ = fl._canvas(2 * HALF, seed)
    window[(start - ((1 << 32) - HALF))[:, None] + np.arange(64)] = fl.frames(g, seed)
    dp.upload(window, (1 << 32) - HALF)
    return dp, (start - data_off).astype(np.uint32), g


def big_who():
    return dict(lo=0, others=[("the buffer's first 64 KiB (a wrapped address)", DECOY_FIRST, 1024)])


@pytest.mark.parametrize("data_off", [0, 4096])
def test_oneshot_imix_offsets_past_4gib(gpu_ctx_factory, monkeypatch, data_off):
    """offsets[i] and data_off are independent u32 values (cop_batch): their
    sum may pass 2^32 and the packet is still at pkts + offsets[i] +
    data_off. At data_off 0 no sum passes 2^32 (offsets end at 0xFFFFFFC0);
    at 4096, 64 packets lie past it, where a 32-bit sum reads the decoy
    frames at the buffer's start. Every address, wrapped or not, is inside
    the one allocation."""
    knobs(monkeypatch)
    ctx, R = make_ctx(gpu_ctx_factory)
    for seed in fl.FILL_SEEDS:
        dp, offs, g = big_slab(ctx, seed, data_off)
        n = len(g)
        assert n == (512 if data_off == 0 else 576) and int(offs.max()) == 0xFFFFFFC0
        assert ((offs.astype(np.int64) + data_off) >= 1 << 32).sum() == (0 if data_off == 0 else 64)
        do = ctx.alloc(n * 4)
        do.upload(offs)
        rec, lst, cnt = (Guarded.packed(ctx, [sz]) for sz in (n * 8, n * 4, 4))
        for x in (rec, lst, cnt):
            x.fill()
        ctx.submit([cg.make_batch(dp, n, rec.addr(), offsets=do, data_off=data_off, fwd_idx=lst.addr(),
                                  fwd_count=cnt.addr())])
        ctx.sync()
        assert ctx.launch_plan() == ("imix", 1), ctx.launch_plan()
        check_batch(f"offsets past 4 GiB, data_off {data_off}", fl.records(g, S | F | L), rec.read("records")[0],
                    lst.read("list")[0], cnt.read("count")[0], **big_who())
        for x in (dp, do, rec.buf, lst.buf, cnt.buf):
            x.free()


@pytest.mark.parametrize("data_off", [0, 4096])
def test_pmd_static_imix_offsets_past_4gib(gpu_ctx_factory, monkeypatch, data_off):
    """The same slab as a one-slot ring of the poll-mode kernel started with
    PMD_STATIC_SLOTS (plain loads; the coherent loads' 2 GiB span check
    refuses such a ring): the IMIX step path's load_step_imix."""
    knobs(monkeypatch)
    ctx, R = make_ctx(gpu_ctx_factory, flags=cg.CFG_SEG_LISTS)
    for seed in fl.FILL_SEEDS:
        dp, offs, g = big_slab(ctx, seed, data_off)
        n = len(g)
        do = ctx.alloc(n * 4)
        do.upload(offs)
        rslot = n + 8
        rec = Guarded.strided(ctx, 1, n * 8, rslot * 8)
        lst = Guarded.strided(ctx, 1, n * 4, (n + 16) * 4)
        cnt = Guarded.strided(ctx, 1, vp.nseg(n) * 4, vp.nseg(n) * 4)
        for x in (rec, lst, cnt):
            x.fill()
        ring = cg.make_ring(dp, 1, n, rec.addr(), BIG, results_slot=rslot, fwd_idx=lst.addr(), fwd_slot=n + 16,
                            fwd_count=cnt.addr(), offsets=do, offsets_slot_words=n, data_off=data_off)
        with ctx.pmd_start(ring, cg.PMD_STATIC_SLOTS) as m:
            assert m.info()["kernel_name"] == "cop_pmd<1, 2, 1, 1, false>", m.info()
            assert m.info()["slot_loads"] == 0
            m.post(1)
            m.wait()
        check_batch(f"poll mode, offsets past 4 GiB, data_off {data_off}", fl.records(g, S | F | L),
                    rec.read("records")[0], lst.read("list")[0], cnt.read("count")[0], seg=True, **big_who())
        for x in (dp, do, rec.buf, lst.buf, cnt.buf):
            x.free()


# ---------------------------------------------------------------------------
# poll mode

# name -> (builder(n, first, seed, R), route, layout argument of the kernel's name)
PMD_LAYOUTS = {
    "coalesced-lds": (lambda n, f, s, R: fl.slots(n, f, s, 64, 0, R), "lds", 2),
    "coalesced-dir": (lambda n, f, s, R: fl.slots(n, f, s, 64, 0, R), "auto", 2),
    "coalesced-bkt": (lambda n, f, s, R: fl.slots(n, f, s, 64, 0, R), "bkt", 2),
    "imix-dir": (lambda n, f, s, R: fl.imix(n, f, s, "phases", 16, R), "auto", 1),
    "imix-bkt": (lambda n, f, s, R: fl.imix(n, f, s, "shuffled", 0, R), "bkt", 1),
    "hdr16": (lambda n, f, s, R: fl.hdr16(n, f, s, R), "auto", 3),
    "wide": (lambda n, f, s, R: fl.slots(n, f, s, 2176, 128, R), "auto", 2),
}
LAP_SHIFT = 3001              # identities of slot s in lap l start at (l * slots + s) * LAP_SHIFT
# (layout, segmented lists): with them the step path where the instantiation has one (tile_steps_v; 16-byte
# records always take the whole-tile body), without them the whole-tile body with dense lists
PMD_CASES = [(k, True) for k in PMD_LAYOUTS] + [("coalesced-lds", False), ("imix-dir", False)]


class LayoutRing:
    """A batch ring whose slots hold layouts of one geometry, outputs guarded."""

    def __init__(self, ctx, lays, seg):
        self.lays, self.seg = list(lays), seg
        P, n = len(lays), len(lays[0].g)
        self.n = n
        self.slot_bytes = -(-max(x.image.nbytes for x in lays) // 256) * 256
        imix = lays[0].offsets is not None
        self.off_words = -(-n // 32) * 32           # offset arrays on 128-byte lines, as the slots
        self.dp = ctx.alloc(P * self.slot_bytes + (P * self.off_words * 4 if imix else 0))
        self.off_at = P * self.slot_bytes
        for s, lay in enumerate(lays):
            self.put(s, lay)
        rslot, fslot = n + 8 + (n & 1), (n + 3) // 4 * 4 + 16
        cw = vp.nseg(n) if seg else 1
        self.rec = Guarded.strided(ctx, P, n * 8, rslot * 8)
        self.lst = Guarded.strided(ctx, P, n * 4, fslot * 4)
        self.cnt = Guarded.strided(ctx, P, cw * 4, cw * 4)
        self.ring = cg.make_ring(self.dp, P, n, self.rec.addr(), self.slot_bytes, results_slot=rslot,
                                 fwd_idx=self.lst.addr(), fwd_slot=fslot, fwd_count=self.cnt.addr(),
                                 offsets=self.dp.addr + self.off_at if imix else None, offsets_slot_words=self.off_words if imix else 0,
                                 **lays[0].kw)

    def put(self, s, lay):
        assert lay.kw == self.lays[0].kw and len(lay.g) == self.n and lay.image.nbytes <= self.slot_bytes
        self.lays[s] = lay
        self.dp.upload(lay.image, s * self.slot_bytes)
        if lay.offsets is not None:
            self.dp.upload(lay.offsets, self.off_at + s * self.off_words * 4)

    def fill(self):
        for x in (self.rec, self.lst, self.cnt):
            x.fill()

    def check(self, what, R, ppt, others):
        r, l, k = self.rec.read("records"), self.lst.read("lists"), self.cnt.read("counts")
        for s, lay in enumerate(self.lays):
            first = fl.span_of(lay.g)
            check_batch(f"{what} slot {s} {lay.name} first={first}", fl.records(lay.g, S | F | L, R), r[s], l[s], k[s],
                        seg=self.seg, lo=max(0, first - fl.WINDOW // 2), first=first, ppt=ppt, R=R,
                        seg_wave=self.seg and ppt == 4, others=[o for o in others if o[1] != first])


@pytest.mark.parametrize("reuse", [False, True], ids=["static", "reused"])
@pytest.mark.parametrize("T", [256, 1024])
@pytest.mark.parametrize("case,seg", PMD_CASES)
def test_pmd_loaders(gpu_ctx_factory, monkeypatch, case, seg, T, reuse):
    """Three laps of a small ring of ragged batches (2T + 259 packets)
    through the poll-mode kernel at 256- and 1024-packet tiles. Static
    slots (PMD_STATIC_SLOTS, plain loads): three slots written once, a
    kernel per filler seed. Reused
    slots (the default: system-coherent loads once the ring has wrapped):
    two slots, rewritten before each lap with the identity frames of a
    shifted index range and the other filler, so a stale read is named as
    the previous lap's packet."""
    build, route, lay_arg = PMD_LAYOUTS[case]
    ppt = T // 256
    knobs(monkeypatch, COP_PPT=ppt, **({"COP_PMD_PER_CU": 4} if T == 256 else {}))
    ctx, R = make_ctx(gpu_ctx_factory, route, flags=cg.CFG_SEG_LISTS if seg else 0)
    n, P = 2 * T + 259, 2 if reuse else 3
    firsts = lambda lap: [(lap * P + s) * LAP_SHIFT for s in range(P)]
    for seed in fl.FILL_SEEDS[:1 if reuse else 2]:      # (reused slots: the laps alternate between the seeds)
        rg = LayoutRing(ctx, [build(n, f, seed, R) for f in firsts(0)], seg)
        with ctx.pmd_start(rg.ring, 0 if reuse else cg.PMD_STATIC_SLOTS) as m:
            info = m.info()
            assert info["kernel_name"] == f"cop_pmd<1, {LPM_ARG[route]}, {lay_arg}, {ppt}, false>", info
            assert info["slot_loads"] == (4 if reuse else 0), info
            for lap in range(3):
                others = [(f"lap {lap} slot {s}", f, n) for s, f in enumerate(firsts(lap if reuse else 0))]
                if reuse and lap:
                    others += [(f"lap {lap - 1} slot {s}", f, n) for s, f in enumerate(firsts(lap - 1))]
                    for s, f in enumerate(firsts(lap)):
                        rg.put(s, build(n, f, fl.FILL_SEEDS[lap % 2], R))
                rg.fill()
                m.post(P)
                m.wait()
                rg.check(f"{case} lap {lap}", R, ppt, others)
            info = m.info()
            assert info["completed"] == 3 * P and info["launches"] == 1, info
