"""GPU: the vport route image (stage P) and the LDS budget ladder at their
edges.

a. Every key of every table of tests/route_cases.py (0, 1, 3, 128, 255 and
   256 leaves; the oracle agrees with the numpy derivation on the host,
   test_route_cases.py) through cop_submit in the four packet layouts at
   256- and 2048-packet tiles, cop_submit_ring, and the poll-mode kernel's
   dense and step paths with slots and IMIX: records, lists and counters.
b. fill_launch's ladder, rung by rung: a launch whose LDS need is exactly
   160 KiB keeps its forms, one 16 bytes larger demotes the route stage to
   its DIR-24-8 image, then the firewall, then fails with -E2BIG. The needs
   A (both stages in LDS), B (route stage DIR-24-8) and C (both) are read
   from cop_debug_launch_forms at $COP_LDS_PAD=0 with the force flags, never
   written down here; the pads follow from them.
c. The hit-bin region of the per-rule counters on both sides of its own
   160 KiB test. d. cop_pmd_start on both sides of the first rung.
e. cop_set_routing_table behind launches in flight and under poll mode.

The table `all` (256 leaves, 129 KiB of image) leaves 31744 bytes: the
fw1k intervals (20496 bytes) fit beside it, a 3000-route table's (73744) or
the trie's top level (16384) do not. So the rungs that keep the route stage
in LDS run on `odd_blocks` (128 leaves), where all six pads exist; `all`
runs the rungs from B on, and at pad 0 already takes the route stage's
DIR-24-8 image.

Every output buffer carries 0xAB guard bytes around its ABI extent.
"""
import errno
import functools
from collections import namedtuple

import numpy as np
import pytest

import copgpu as cg
import oracle as orc
import route_cases as rc
import verdict_patterns as vp
from helpers import oracle_tables

pytestmark = pytest.mark.gpu

S, F, L = rc.S, rc.F, rc.L
N, K = rc.N, rc.N_PORTS
SEG = vp.SEG
LIM = 160 * 1024          # gfx950 LDS per workgroup: the limit of fill_launch's ladder
GUARD = 64
KNOBS = ("COP_PPT", "COP_LDS_PAD", "COP_HIT_BINS", "COP_STATIC_ORDER", "COP_STAGE_LISTS", "COP_REC_PAIRED", "COP_TBL8",
         "COP_LOADS", "COP_PMD_REC", "COP_PMD_DYN", "COP_PMD_PF", "COP_PMD_IDLE_MS", "COP_PMD_PER_CU")


def knobs(monkeypatch, **kv):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, str(v))


# ---------------------------------------------------------------------------
# outputs

class Guarded:
    """One device buffer of `count` extents of `size` bytes, `stride` apart,
    every other byte of it a guard."""

    def __init__(self, ctx, count, size, stride=None):
        stride = size if stride is None else stride
        assert stride >= size
        self.extents = [(GUARD + s * stride, size) for s in range(count)]
        total = GUARD + count * stride + GUARD
        self.buf = ctx.alloc(total)
        self.inside = np.zeros(total, dtype=bool)
        for o, sz in self.extents:
            self.inside[o:o + sz] = True

    def addr(self, k=0):
        return self.buf.addr + self.extents[k][0]

    def fill(self):
        self.buf.fill(0xAB)

    def raw(self):
        return self.buf.download(np.uint8, self.buf.nbytes)

    def read(self, what):
        raw = self.raw()
        bad = np.nonzero(~self.inside & (raw != 0xAB))[0]
        assert bad.size == 0, f"{what}: guard bytes overwritten at {bad[:8]}"
        return [raw[o:o + sz] for o, sz in self.extents]

    def free(self):
        self.buf.free()


class Outputs:
    """Records, lists and counts of P batches of N packets (ring slots when
    P > 1), guarded."""

    def __init__(self, ctx, mode, P=1):
        self.mode, self.P = mode, P
        self.rslot = N + 8                                       # even: records may go out from lane pairs
        self.words = N * K if mode == "demux" else N
        self.fslot = (self.words + 3) // 4 * 4 + 16
        self.cw = {"dense": 1, "seg": vp.nseg(N), "demux": K}[mode]
        self.rec = Guarded(ctx, P, N * 8, self.rslot * 8)
        self.lst = Guarded(ctx, P, self.words * 4, self.fslot * 4)
        self.cnt = Guarded(ctx, P, self.cw * 4)                  # counts are contiguous
        self.fill()

    def fill(self):
        for g in (self.rec, self.lst, self.cnt):
            g.fill()

    def batch(self, dp, stride=64, offsets=None):
        return cg.make_batch(dp, N, self.rec.addr(), stride=stride or 64, offsets=offsets, fwd_idx=self.lst.addr(),
                             fwd_count=self.cnt.addr())

    def ring(self, dp, slot_bytes, **kw):
        return cg.make_ring(dp, self.P, N, self.rec.addr(), slot_bytes, results_slot=self.rslot,
                            fwd_idx=self.lst.addr(), fwd_slot=self.fslot, fwd_count=self.cnt.addr(), **kw)

    def check(self, e, what, slots=None):
        r, l, k = self.rec.read(what + ": records"), self.lst.read(what + ": lists"), self.cnt.read(what + ": counts")
        for s in range(self.P) if slots is None else slots:
            check_batch(e, self.mode, r[s], l[s], k[s], f"{what}, slot {s}")

    def untouched(self):
        return all((g.raw() == 0xAB).all() for g in (self.rec, self.lst, self.cnt))

    def free(self):
        for g in (self.rec, self.lst, self.cnt):
            g.free()


def check_batch(e, mode, rec, lst, cnt, what):
    got = rec.view(cg.RESULT_DT)
    for f in ("verdict", "flags", "port", "route_nh"):
        bad = np.nonzero(got[f] != e.rec[f])[0]
        assert bad.size == 0, f"{what}: {f} at {bad[:8]}: gpu {got[f][bad[:8]]}, expected {e.rec[f][bad[:8]]}"
    lst, cnt = lst.view(np.uint32), cnt.view(np.uint32)
    if mode == "dense":
        want = vp.dense_list(e.fwd)
        assert cnt[0] == len(want), f"{what}: count {cnt[0]}, expected {len(want)}"
        assert np.array_equal(lst[:len(want)], want), f"{what}: dense list"
    elif mode == "seg":
        wc, wl = vp.seg_lists(e.fwd)
        assert np.array_equal(cnt, wc), f"{what}: segment counts"
        for s, w in enumerate(wl):
            assert np.array_equal(lst[s * SEG:s * SEG + len(w)], w), f"{what}: segment {s}"
    else:
        wc, wl = rc.port_lists(e)
        assert np.array_equal(cnt, wc), f"{what}: port counts {cnt}, expected {wc}"
        for q, w in enumerate(wl):
            assert np.array_equal(lst[q * N:q * N + len(w)], w), f"{what}: port {q} list"


def check_counters(ctx, e, reps=1):
    got = ctx.counters()
    assert got == {k: reps * v for k, v in e.cnt.items()}, (got, e.cnt, reps)


def upload(ctx, layout):
    """(device buffer, stride, device offsets or None) of the frames in a layout."""
    data, stride, offs = layout
    dp = ctx.alloc(data.nbytes + (offs.nbytes if offs is not None else 0))
    dp.upload(data)
    if offs is not None:
        dp.upload(offs, data.nbytes)
    return dp, stride, (dp.addr + data.nbytes) if offs is not None else None


def oneshot(ctx, layout, e, mode, what):
    dp, stride, doff = upload(ctx, layout)
    out = Outputs(ctx, mode)
    ctx.counters(reset=True)
    ctx.submit([out.batch(dp, stride, doff)])
    ctx.sync()
    out.check(e, what)
    check_counters(ctx, e)
    out.free()
    dp.free()


def slot_bytes(layout):
    data, _, offs = layout
    return (data.nbytes + (offs.nbytes if offs is not None else 0) + 4095) // 4096 * 4096


def ring_of(ctx, layout, mode, P):
    """A ring of P slots that all hold the frames of `layout`."""
    data, stride, offs = layout
    per = slot_bytes(layout)
    dp = ctx.alloc(per * P)
    for s in range(P):
        dp.upload(data, s * per)
        if offs is not None:
            dp.upload(offs, s * per + data.nbytes)
    out = Outputs(ctx, mode, P)
    kw = {} if offs is None else dict(offsets=dp.addr + data.nbytes, offsets_slot_words=per // 4)
    return dp, out, out.ring(dp, per, **kw)


# ---------------------------------------------------------------------------
# a. every key, every table, every path

def small_ctx(factory, name, flags=0):
    """The tiny firewall and route tables of verdict_patterns.py beside the
    named routing table: everything stays in LDS."""
    ctx = factory(stages=S | F | L, n_ports=K, flags=flags, routing_table=rc.table(name))
    ctx.set_fw_table(cg.LpmTable(vp.fw_rules(), *vp.FW_CFG))
    ctx.set_route_lpm(cg.LpmTable(vp.route_rules(), 1 << 20, 1 << 16, False))
    return ctx


@functools.lru_cache(maxsize=None)
def small_expected(name):
    return rc.expected(rc.table(name), S | F | L)


@pytest.mark.parametrize("ppt", [1, 8])
@pytest.mark.parametrize("name", list(rc.TABLES))
def test_submit_every_key(gpu_ctx_factory, monkeypatch, name, ppt):
    knobs(monkeypatch, COP_PPT=ppt)
    ctx = small_ctx(gpu_ctx_factory, name)
    e = small_expected(name)
    for lay in rc.LAYOUTS:
        oneshot(ctx, rc.layout(lay), e, "dense", f"{name}/{lay}/ppt={ppt}")
        fw, rt, lds = ctx.launch_forms()
        assert (fw, rt) == ("lds", "lds") and lds <= LIM, (fw, rt, lds)


@pytest.mark.parametrize("name", list(rc.TABLES))
def test_submit_ring_every_key(gpu_ctx_factory, monkeypatch, name):
    knobs(monkeypatch)
    ctx = small_ctx(gpu_ctx_factory, name)
    e = small_expected(name)
    dp, out, ring = ring_of(ctx, rc.layout("slots"), "dense", 2)
    ctx.counters(reset=True)
    ctx.submit_ring(ring, 1, 2)            # slots 1, 0
    ctx.sync()
    out.check(e, name)
    check_counters(ctx, e, reps=2)


@pytest.mark.parametrize("mode", ["dense", "seg"])
@pytest.mark.parametrize("name", list(rc.TABLES))
def test_pmd_every_key(gpu_ctx_factory, monkeypatch, name, mode):
    """The poll-mode kernel's dense path (tile_body) and step path
    (segmented lists), 1024-packet tiles, slots and IMIX."""
    knobs(monkeypatch)
    ctx = small_ctx(gpu_ctx_factory, name, flags=cg.CFG_SEG_LISTS if mode == "seg" else 0)
    e = small_expected(name)
    for lay in ("slots", "imix"):
        dp, out, ring = ring_of(ctx, rc.layout(lay), mode, 2)
        ctx.counters(reset=True)
        with ctx.pmd_start(ring) as m:
            info = m.info()
            assert (info["kernel"] & 0xFF) == 0x11 and info["packets_per_tile"] == 1024, info
            m.post(2)
            m.wait()
            out.check(e, f"{name}/{lay}/{mode}")
        check_counters(ctx, e, reps=2)
        out.free()
        dp.free()


@pytest.mark.parametrize("ppt", [1, 8])
@pytest.mark.parametrize("name", ["odd_blocks", "all"])
def test_demux_every_key(gpu_ctx_factory, monkeypatch, name, ppt):
    """DEMUX_PORTS | PORT_STATS on the dense tables' ports 0..4: one list per
    vport and the per-port statistics (the EXT kernel's wider misc carve)."""
    knobs(monkeypatch, COP_PPT=ppt)
    ctx = small_ctx(gpu_ctx_factory, name, flags=cg.CFG_DEMUX_PORTS | cg.CFG_PORT_STATS)
    e = small_expected(name)
    ctx.port_stats(reset=True)
    oneshot(ctx, rc.layout("slots"), e, "demux", f"{name}/demux/ppt={ppt}")
    ps = ctx.port_stats()
    got = np.array([[ps[q]["rx_packets"], ps[q]["tx_packets"]] for q in range(K)])
    assert np.array_equal(got, rc.port_stats(e)), (got, rc.port_stats(e))
    assert all(ps[q]["nf_dropped"] == ps[q]["rx_packets"] - ps[q]["tx_packets"] for q in range(K))


# ---------------------------------------------------------------------------
# b. the ladder, rung by rung

def fw1k():
    return cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)


def routes(n):
    return cg.gen_rules(0x5EED2003, n, cg.GEN_ROUTES, 0)


@functools.lru_cache(maxsize=None)
def ladder_frames(n_routes=3000):
    """The generator's traffic for the fw1k rules and the route table, its
    destinations' low 16 bits replaced by route_cases' keys (every key once,
    then the parse-stage tail)."""
    fr = rc.frames()
    pk = cg.gen_trace(0x5EED7C00 + n_routes, N, fw1k(), routes(n_routes),
                      opts=cg.trace_opts(pct_non_ipv4=0, pct_bad_version=0, pct_unknown_dst=0))
    f = pk.reshape(N, 64)
    f[:, 32] = fr.key >> 8
    f[:, 33] = fr.key & 0xFF
    f[~fr.eth_ok, 12:14] = (0x86, 0xDD)
    f[~fr.ver_ok, 14] = 0x65
    pk.setflags(write=False)
    return pk


Ladder = namedtuple("Ladder", "rec fwd cnt hits")


@functools.lru_cache(maxsize=None)
def ladder_expected(name, n_routes=3000):
    """The oracle on ladder_frames under the named routing table."""
    fwo, rto = oracle_tables(fw1k(), routes(n_routes))
    hits = np.zeros(fwo.n_rules, np.uint64)
    ro, fo, co = orc.process(ladder_frames(n_routes), N, rt=rc.table(name), n_ports=K, stages=S | F | L, fw=fwo,
                             route=rto, rule_hits=hits)
    fwd = ro["verdict"] == cg.FORWARD
    assert np.array_equal(fo, vp.dense_list(fwd))
    assert hits.sum() > 4096 and np.count_nonzero(hits) > 500 and (ro["flags"] & cg.FLAG_ROUTE_HIT).sum() > 1024
    for a in (ro, fwd, hits):
        a.setflags(write=False)
    return Ladder(ro, fwd, co, hits)


def ladder_ctx(factory, name, flags=0, n_routes=3000, **kw):
    ctx = factory(stages=S | F | L, n_ports=K, flags=flags, routing_table=rc.table(name), **kw)
    ctx.set_fw_table(cg.LpmTable(fw1k(), 1024, 24, True))
    ctx.set_route_lpm(cg.LpmTable(routes(n_routes), 1 << 20, 1 << 16, False))
    return ctx


def ladder_launch(ctx, name, mode="dense", n_routes=3000):
    """One cop_submit of the ladder frames, checked against the oracle;
    returns launch_forms()."""
    oneshot(ctx, (ladder_frames(n_routes), 64, None), ladder_expected(name, n_routes), mode, f"ladder/{name}")
    return ctx.launch_forms()


def list_mode(flags):
    return "seg" if flags & cg.CFG_SEG_LISTS else "demux" if flags & cg.CFG_DEMUX_PORTS else "dense"


_PROBED = {}
FORCE = {"A": 0, "B": cg.CFG_LPM_FORCE_DIR24, "C": cg.CFG_LPM_FORCE_DIR24 | cg.CFG_FW_FORCE_DIR24}


def probe(factory, monkeypatch, name, which, flags=0, n_routes=3000, **env):
    """The LDS bytes of a launch at $COP_LDS_PAD=0 with the force flags of
    rung `which`: a measurement of the layout, not an expectation."""
    key = (name, which, flags, n_routes, tuple(sorted(env.items())))
    if key not in _PROBED:
        knobs(monkeypatch, COP_LDS_PAD=0, **env)
        ctx = ladder_ctx(factory, name, flags | FORCE[which], n_routes)
        fw, rt, lds = ladder_launch(ctx, name, list_mode(flags), n_routes)
        print(f"probe {name} {which} flags={flags:#x} routes={n_routes} {env}: {fw}/{rt} {lds} bytes")
        want_rt = "dir" if which != "A" else ("trie" if flags & cg.CFG_LPM_TRIE else "lds")
        assert (fw, rt) == ("dir" if which == "C" else "lds", want_rt), (name, which, fw, rt, lds)
        assert lds % 16 == 0
        _PROBED[key] = lds
        ctx.close()
    return _PROBED[key]


RUNGS = [("A", 0, "lds", "lds"), ("A", 16, "lds", "dir"), ("B", 0, "lds", "dir"), ("B", 16, "dir", "dir"),
         ("C", 0, "dir", "dir"), ("C", 16, None, None)]
# `all` leaves no room for the route intervals at any pad: its rungs start at B
LADDER_CASES = [("odd_blocks", r) for r in RUNGS] + [("all", r) for r in RUNGS[2:]]


@pytest.mark.parametrize("name,rung", LADDER_CASES, ids=[f"{n}-{r[0]}+{r[1]}" for n, r in LADDER_CASES])
def test_ladder_rungs(gpu_ctx_factory, monkeypatch, name, rung):
    """pad = LIM - X: the launch needs exactly 160 KiB and keeps the forms of
    X; 16 bytes more and the next stage is demoted (route first), and past
    the last rung cop_submit returns -E2BIG and writes nothing."""
    which, over, want_fw, want_rt = rung
    X = probe(gpu_ctx_factory, monkeypatch, name, which, COP_PPT=1)
    assert X <= LIM, (name, which, X)
    pad = LIM - X + over
    knobs(monkeypatch, COP_PPT=1, COP_LDS_PAD=pad)
    ctx = ladder_ctx(gpu_ctx_factory, name)
    if want_fw is not None:
        fw, rt, lds = ladder_launch(ctx, name)
        print(f"ladder {name}: {which} = {X}, pad {pad}: {fw}/{rt}, {lds} bytes")
        assert (fw, rt) == (want_fw, want_rt), (pad, fw, rt, lds)
        assert lds <= LIM
        if over == 0:
            assert lds == LIM, (pad, lds)
        return
    dp, stride, _ = upload(ctx, (ladder_frames(), 64, None))
    out = Outputs(ctx, "dense")
    with pytest.raises(cg.CopError) as ei:
        ctx.submit([out.batch(dp)])
    assert ei.value.code == -errno.E2BIG and "LDS" in str(ei.value), ei.value
    ctx.sync()
    assert out.untouched()
    assert ctx.launch_forms() is None
    assert ctx.counters()["rx"] == 0


def test_dense_table_takes_the_route_image_at_pad_zero(gpu_ctx_factory, monkeypatch):
    """256 leaves beside the fw1k and 3000-route intervals need more than
    160 KiB without any pad: the first launch already demotes the route
    stage, and only it."""
    knobs(monkeypatch, COP_PPT=1)
    ctx = ladder_ctx(gpu_ctx_factory, "all")
    assert ctx.route_form() == "lds"                 # the table's own form; the launch decides
    fw, rt, lds = ladder_launch(ctx, "all")
    assert (fw, rt) == ("lds", "dir") and lds == probe(gpu_ctx_factory, monkeypatch, "all", "B", COP_PPT=1)


@pytest.mark.parametrize("over,want_rt", [(0, "lds"), (16, "dir")])
@pytest.mark.parametrize("flags", [cg.CFG_PORT_STATS, cg.CFG_DEMUX_PORTS | cg.CFG_PORT_STATS], ids=["stats", "demux"])
def test_ladder_first_rung_with_the_wider_misc_carve(gpu_ctx_factory, monkeypatch, flags, over, want_rt):
    """PORT_STATS and DEMUX_PORTS take the EXT kernel's misc words (and demux
    no list stage): the first rung sits where their own need says."""
    name = "odd_blocks"
    A = probe(gpu_ctx_factory, monkeypatch, name, "A", flags=flags, COP_PPT=1)
    A0 = probe(gpu_ctx_factory, monkeypatch, name, "A", COP_PPT=1)
    assert A != A0, (A, A0)
    pad = LIM - A + over
    knobs(monkeypatch, COP_PPT=1, COP_LDS_PAD=pad)
    ctx = ladder_ctx(gpu_ctx_factory, name, flags)
    ctx.port_stats(reset=True)
    fw, rt, lds = ladder_launch(ctx, name, list_mode(flags))
    print(f"ladder flags {flags:#x}: A = {A}, pad {pad}: {fw}/{rt}, {lds} bytes")
    assert (fw, rt) == ("lds", want_rt), (pad, fw, rt, lds)
    assert lds == LIM if over == 0 else lds < LIM
    e = ladder_expected(name)
    ps = ctx.port_stats()
    got = np.array([[ps[q]["rx_packets"], ps[q]["tx_packets"]] for q in range(K)])
    assert np.array_equal(got, rc.port_stats(e)), (got, rc.port_stats(e))


@pytest.mark.parametrize("over,want_rt", [(0, "trie"), (16, "dir")])
def test_ladder_trie_falls_back_to_dir(gpu_ctx_factory, monkeypatch, over, want_rt):
    """The route table in the trie form (20k routes, 16 KiB top level in
    LDS): at the limit it stays, 16 bytes over it is looked up in the
    DIR-24-8 image."""
    name, nr = "odd_blocks", 20000
    A = probe(gpu_ctx_factory, monkeypatch, name, "A", flags=cg.CFG_LPM_TRIE, n_routes=nr, COP_PPT=1)
    pad = LIM - A + over
    knobs(monkeypatch, COP_PPT=1, COP_LDS_PAD=pad)
    ctx = ladder_ctx(gpu_ctx_factory, name, cg.CFG_LPM_TRIE, nr)
    assert ctx.route_form() == "trie"
    fw, rt, lds = ladder_launch(ctx, name, n_routes=nr)
    print(f"ladder trie: A = {A}, pad {pad}: {fw}/{rt}, {lds} bytes")
    assert (fw, rt) == ("lds", want_rt), (pad, fw, rt, lds)
    assert lds == LIM if over == 0 else lds < LIM


def test_ladder_wider_tile_crosses_alone(gpu_ctx_factory, monkeypatch):
    """Segmented lists on one pad, the 256-packet tile's need exactly at the
    limit: the 2048-packet tile's list stage (7 KiB more) crosses it. The
    forms differ, the records and lists do not."""
    name = "odd_blocks"
    A1 = probe(gpu_ctx_factory, monkeypatch, name, "A", flags=cg.CFG_SEG_LISTS, COP_PPT=1)
    # the wider tile's need, measured where it fits (the route stage forced to DIR-24-8)
    B1 = probe(gpu_ctx_factory, monkeypatch, name, "B", flags=cg.CFG_SEG_LISTS, COP_PPT=1)
    B8 = probe(gpu_ctx_factory, monkeypatch, name, "B", flags=cg.CFG_SEG_LISTS, COP_PPT=8)
    assert B8 - B1 == 7 * 256 * 4, (B1, B8)          # the list stage: 256 * ppt words
    A8 = A1 + B8 - B1
    pad = LIM - A1
    got = {}
    for ppt in (1, 8):
        knobs(monkeypatch, COP_PPT=ppt, COP_LDS_PAD=pad)
        ctx = ladder_ctx(gpu_ctx_factory, name, cg.CFG_SEG_LISTS)
        got[ppt] = ladder_launch(ctx, name, "seg")
    print(f"ladder seg: A(256) = {A1}, A(2048) = {A8}, pad {pad}: {got}")
    assert got[1] == ("lds", "lds", LIM), got
    assert got[8][:2] == ("lds", "dir") and got[8][2] <= LIM, got


# ---------------------------------------------------------------------------
# c. rule counters at the limit

def hit_bin_sides(factory, monkeypatch, name, pmd=False):
    """(B, H): a launch's LDS bytes at pad 0 with the route stage in its
    DIR-24-8 image, without and with the hit-bin region."""
    B = probe(factory, monkeypatch, name, "B", flags=cg.CFG_RULE_COUNTERS, COP_PPT=1, COP_HIT_BINS=0)
    H = probe(factory, monkeypatch, name, "B", flags=cg.CFG_RULE_COUNTERS, COP_PPT=1, COP_HIT_BINS=1)
    assert B < H <= LIM, (B, H)
    return B, H


@pytest.mark.parametrize("over", [0, 16])
def test_rule_counters_on_both_sides_of_the_hit_bin_limit(gpu_ctx_factory, monkeypatch, over):
    """$COP_HIT_BINS=1 with the hit-bin region ending exactly at 160 KiB
    (binned) and 16 bytes past it (one atomic per hit): the same per-rule
    counts, the oracle's."""
    name = "all"
    B, H = hit_bin_sides(gpu_ctx_factory, monkeypatch, name)
    pad = LIM - H + over
    knobs(monkeypatch, COP_PPT=1, COP_HIT_BINS=1, COP_LDS_PAD=pad)
    ctx = ladder_ctx(gpu_ctx_factory, name, cg.CFG_RULE_COUNTERS)
    ctx.rule_counters(reset=True)
    fw, rt, lds = ladder_launch(ctx, name)
    print(f"hit bins: B = {B}, with bins {H}, pad {pad}: {fw}/{rt}, {lds} bytes")
    assert (fw, rt) == ("lds", "dir")
    assert lds == (LIM if over == 0 else B + pad), (pad, lds)      # binned, or the carve without the region
    want = ladder_expected(name).hits
    got = ctx.rule_counters()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


@pytest.mark.parametrize("over", [0, 16])
def test_pmd_rule_counters_on_both_sides_of_the_hit_bin_limit(gpu_ctx_factory, monkeypatch, over):
    """The same under the poll-mode kernel with one ring (its own carve, read
    from the started kernel at pad 0)."""
    name = "all"
    e = ladder_expected(name)
    sides = {}
    for bins in (0, 1):
        knobs(monkeypatch, COP_PPT=1, COP_PMD_PER_CU=4, COP_HIT_BINS=bins, COP_LDS_PAD=0)
        ctx = ladder_ctx(gpu_ctx_factory, name, cg.CFG_RULE_COUNTERS)
        dp, out, ring = ring_of(ctx, (ladder_frames(), 64, None), "dense", 1)
        with ctx.pmd_start(ring) as m:
            sides[bins] = m.launch_forms()
        out.free()
        dp.free()
        ctx.close()
    assert sides[0][:2] == sides[1][:2] == ("lds", "dir") and sides[0][2] < sides[1][2] <= LIM, sides
    Bp, Hp = sides[0][2], sides[1][2]
    pad = LIM - Hp + over
    knobs(monkeypatch, COP_PPT=1, COP_PMD_PER_CU=4, COP_HIT_BINS=1, COP_LDS_PAD=pad)
    ctx = ladder_ctx(gpu_ctx_factory, name, cg.CFG_RULE_COUNTERS)
    dp, out, ring = ring_of(ctx, (ladder_frames(), 64, None), "dense", 2)
    ctx.counters(reset=True)
    ctx.rule_counters(reset=True)
    with ctx.pmd_start(ring) as m:
        fw, rt, lds = m.launch_forms()
        print(f"pmd hit bins: B' = {Bp}, with bins {Hp}, pad {pad}: {fw}/{rt}, {lds} bytes")
        assert (fw, rt) == ("lds", "dir") and lds == (LIM if over == 0 else Bp + pad), (pad, fw, rt, lds)
        assert m.info()["workers_per_cu"] >= 1
        m.post(2)
        m.wait()
        out.check(e, "pmd rule counters")
    check_counters(ctx, e, reps=2)
    got = ctx.rule_counters()
    assert np.array_equal(got, 2 * e.hits), np.nonzero(got != 2 * e.hits)[0][:10]


# ---------------------------------------------------------------------------
# d. poll mode under the ladder

@pytest.mark.parametrize("over,want_rt", [(0, 1), (16, 2)])
def test_pmd_on_both_sides_of_the_first_rung(gpu_ctx_factory, monkeypatch, over, want_rt):
    """cop_pmd_start goes through the same ladder. A' (read from a kernel
    started at pad 0, cop_debug_pmd_forms) puts its need exactly at 160 KiB
    and 16 bytes over: route form 1 (LDS), then 2 (DIR-24-8), at least one
    worker per CU resident either way, and three posts around a 4-slot ring
    complete with the oracle's records, lists and counters."""
    name = "odd_blocks"
    e = ladder_expected(name)
    key = ("pmd", name)
    if key not in _PROBED:
        knobs(monkeypatch, COP_PPT=1, COP_PMD_PER_CU=4, COP_LDS_PAD=0)
        ctx = ladder_ctx(gpu_ctx_factory, name)
        dp, out, ring = ring_of(ctx, (ladder_frames(), 64, None), "dense", 1)
        with ctx.pmd_start(ring) as m:
            fw, rt, lds = m.launch_forms()
        assert (fw, rt) == ("lds", "lds") and lds % 16 == 0, (fw, rt, lds)
        _PROBED[key] = lds
        out.free()
        dp.free()
        ctx.close()
    Ap = _PROBED[key]
    pad = LIM - Ap + over
    knobs(monkeypatch, COP_PPT=1, COP_PMD_PER_CU=4, COP_LDS_PAD=pad)
    ctx = ladder_ctx(gpu_ctx_factory, name)
    P = 4
    dp, out, ring = ring_of(ctx, (ladder_frames(), 64, None), "dense", P)
    ctx.counters(reset=True)
    with ctx.pmd_start(ring) as m:
        info = m.info()
        fw, rt, lds = m.launch_forms()
        print(f"pmd ladder: A' = {Ap}, pad {pad}: kernel {info['kernel']:#x}, {lds} bytes, "
              f"{info['workers_per_cu']} per CU")
        assert (info["kernel"] & 15) == 1 and ((info["kernel"] >> 4) & 15) == want_rt, info
        assert info["workers_per_cu"] >= 1 and info["packets_per_tile"] == 256, info
        assert lds == LIM if over == 0 else lds <= LIM
        done = 0
        for lap in range(3):
            out.fill()
            m.post(3)
            m.wait()
            out.check(e, f"post {lap}", slots=[(done + k) % P for k in range(3)])
            done += 3
        assert m.info()["completed"] == 9
    check_counters(ctx, e, reps=9)


# ---------------------------------------------------------------------------
# e. cop_set_routing_table after create

@pytest.mark.parametrize("n_streams", [1, 3])
def test_set_routing_table_behind_launches_in_flight(gpu_ctx_factory, monkeypatch, n_streams):
    """Three submits of one batch with the table swapped between them and no
    sync by the caller: each launch sees the table that was current when it
    was submitted (`uniform`, `all`, `uniform`), and the LDS carve follows
    the leaf count (the route stage moves to its DIR-24-8 image and back)."""
    knobs(monkeypatch, COP_PPT=1)
    ctx = ladder_ctx(gpu_ctx_factory, "uniform", n_streams=n_streams)
    dp, stride, _ = upload(ctx, (ladder_frames(), 64, None))
    seq = [("uniform", "lds"), ("all", "dir"), ("uniform", "lds")]
    outs, forms = [], []
    ctx.counters(reset=True)
    for i, (name, _) in enumerate(seq):
        if i:
            ctx.set_routing_table(rc.table(name))
        outs.append(Outputs(ctx, "dense"))
        ctx.submit([outs[-1].batch(dp)])
        forms.append(ctx.launch_forms())
    ctx.sync()
    for (name, want_rt), out, (fw, rt, lds) in zip(seq, outs, forms):
        out.check(ladder_expected(name), f"table {name}")
        assert (fw, rt) == ("lds", want_rt) and lds <= LIM, (name, fw, rt, lds)
    assert forms[0][2] == forms[2][2] and forms[1][2] - forms[0][2] == \
        256 * 512 - (2 * 8192 + 2052) * 4                       # + 256 leaves, - the route intervals (m = 8192)
    want = vp.add_counters(*[ladder_expected(name).cnt for name, _ in seq])
    assert ctx.counters() == want
    assert cg.lib().cop_set_routing_table(ctx.handle, None) == -errno.EINVAL


def test_set_routing_table_under_poll_mode(gpu_ctx_factory, monkeypatch):
    """-EBUSY while a poll-mode kernel serves the context, whose next batch
    still sees the old table; after the stop the call succeeds and a
    one-shot launch sees the new one."""
    knobs(monkeypatch, COP_PPT=1, COP_PMD_PER_CU=4)
    ctx = ladder_ctx(gpu_ctx_factory, "uniform")
    dp, out, ring = ring_of(ctx, (ladder_frames(), 64, None), "dense", 2)
    with ctx.pmd_start(ring) as m:
        m.post(1)
        m.wait()
        with pytest.raises(cg.CopError) as ei:
            ctx.set_routing_table(rc.table("all"))
        assert ei.value.code == -errno.EBUSY, ei.value
        m.post(1)
        m.wait()
        out.check(ladder_expected("uniform"), "under poll mode")
    ctx.set_routing_table(rc.table("all"))
    assert ladder_launch(ctx, "all")[:2] == ("lds", "dir")
