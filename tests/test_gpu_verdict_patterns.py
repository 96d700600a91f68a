"""GPU: forward-list compaction, record stores and counters on prescribed
verdict patterns.

Every batch here is built so that each packet's verdict class and vport are
prescribed (tests/verdict_patterns.py; the oracle agrees with the
prescription on the host, test_verdict_patterns.py), so the records, the
dense / segmented / per-port forward lists, the nine counters, the port
statistics and the per-rule hits follow from the prescription by plain
numpy. The patterns put the code after the verdicts on its edges: tiles,
segments, waves and 16-byte chunks whose forward count is 0, 1, full or a
given residue mod 4, a lone forward in lane 0 or lane 63, whole tiles that
drop, look-back chains whose predecessors all publish aggregate 0, and a
chain of 258 tiles (a second look-back round). They run through the
one-shot kernel at every tile size, tile order and list form, and through
the poll-mode kernel's step path, dense path and EXT instantiations.

Every output buffer carries 0xAB guard bytes before and after its ABI
extent (n records; n list words, or K * n with demux; 1, ceil(n / 256) or K
counts): the guards must be untouched. Nothing is asserted about list words
between a list's length and its extent.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import copgpu as cg
import verdict_patterns as vp

pytestmark = pytest.mark.gpu

S, F, L = vp.S, vp.F, vp.L
SEG = vp.SEG
GUARD = 64        # guard bytes around every extent
KNOBS = ("COP_PPT", "COP_STATIC_ORDER", "COP_STAGE_LISTS", "COP_REC_PAIRED", "COP_HIT_BINS", "COP_TBL8",
         "COP_LOADS", "COP_PMD_REC", "COP_PMD_DYN", "COP_PMD_PF", "COP_PMD_IDLE_MS", "COP_PMD_PER_CU")

Case = namedtuple("Case", "name n fwd cl ports pk rec cnt")


def knobs(monkeypatch, **kv):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, str(v))


@functools.lru_cache(maxsize=None)
def masks(n, T):
    return vp.patterns(n, T)


@functools.lru_cache(maxsize=None)
def case(name, n, T, K=5, layout="mod", lpm=False):
    """One batch: computed once, shared, read-only."""
    fwd = masks(n, T)[name]
    cl = vp.classes_of(name, fwd)
    ports = vp.port_layouts(n, T, K)[layout]
    pk, rec, cnt = vp.frames(cl, ports, route_hit=vp.route_hit_mask(n) if lpm else None,
                             stages=S | F | L if lpm else S | F)
    for a in (cl, ports, pk, rec):
        a.setflags(write=False)
    return Case(f"{name}/{layout}/n={n}", n, fwd, cl, ports, pk, rec, cnt)


def cases(n, T, names=None, **kw):
    return [case(name, n, T, **kw) for name in (names if names is not None else masks(n, T))]


def make_ctx(factory, K=5, flags=0, stages=S | F):
    ctx = factory(stages=stages, n_ports=K, flags=flags, routing_table=vp.routing_table(K))
    ctx.set_fw_table(cg.LpmTable(vp.fw_rules(), *vp.FW_CFG))
    if stages & L:
        ctx.set_route_lpm(cg.LpmTable(vp.route_rules(), 1 << 20, 1 << 16, False))
        assert ctx.route_form() == "lds"
    return ctx


class Guarded:
    """One device buffer holding several output extents (byte offset, byte
    size), every other byte of it a guard."""

    def __init__(self, ctx, extents, total):
        self.extents = extents
        self.buf = ctx.alloc(total)
        self.inside = np.zeros(total, dtype=bool)
        for o, sz in extents:
            assert GUARD <= o and o + sz + GUARD <= total
            self.inside[o:o + sz] = True

    @classmethod
    def packed(cls, ctx, sizes, align=16, shift=0):
        """Extents of the given sizes, each starting `shift` bytes past an
        `align` boundary, GUARD or more bytes apart."""
        ext, cur = [], 0
        for sz in sizes:
            o = -(-(cur + GUARD) // align) * align + shift
            ext.append((o, sz))
            cur = o + sz
        return cls(ctx, ext, cur + GUARD + align)

    @classmethod
    def strided(cls, ctx, count, size, stride):
        """`count` extents `stride` bytes apart (ring slots)."""
        assert stride >= size
        return cls(ctx, [(GUARD + s * stride, size) for s in range(count)], GUARD + count * stride + GUARD)

    def addr(self, k=0):
        return self.buf.addr + self.extents[k][0]

    def fill(self):
        self.buf.fill(0xAB)

    def read(self, what):
        raw = self.buf.download(np.uint8, self.buf.nbytes)
        bad = np.nonzero(~self.inside & (raw != 0xAB))[0]
        assert bad.size == 0, f"{what}: guard bytes overwritten at {bad[:8]} (extents {self.extents[:4]} ...)"
        return [raw[o:o + sz] for o, sz in self.extents]


def list_words(n, mode, K):
    return n * K if mode == "demux" else n


def count_words(n, mode, K):
    return {"dense": 1, "seg": vp.nseg(n), "demux": K}[mode]


def check_case(c, mode, K, rec, lst, cnt):
    """One batch's records, lists and counts against its prescription."""
    got = rec.view(cg.RESULT_DT)
    for f in ("verdict", "flags", "port", "route_nh"):
        bad = np.nonzero(got[f] != c.rec[f])[0]
        assert bad.size == 0, f"{c.name}: {f} at {bad[:8]}: gpu {got[f][bad[:8]]}, prescribed {c.rec[f][bad[:8]]}"
    lst, cnt = lst.view(np.uint32), cnt.view(np.uint32)
    if mode == "dense":
        want = vp.dense_list(c.fwd)
        assert cnt[0] == len(want), f"{c.name}: count {cnt[0]}, prescribed {len(want)}"
        assert np.array_equal(lst[:len(want)], want), f"{c.name}: dense list"
    elif mode == "seg":
        wc, wl = vp.seg_lists(c.fwd)
        assert np.array_equal(cnt, wc), f"{c.name}: segment counts {cnt[:8]}, prescribed {wc[:8]}"
        for s, w in enumerate(wl):
            assert np.array_equal(lst[s * SEG:s * SEG + len(w)], w), f"{c.name}: segment {s} (length {len(w)})"
    else:
        wc, wl = vp.port_lists(c.fwd, c.ports, K)
        assert np.array_equal(cnt, wc), f"{c.name}: port counts {cnt}, prescribed {wc}"
        for q, w in enumerate(wl):
            assert np.array_equal(lst[q * c.n:q * c.n + len(w)], w), f"{c.name}: port {q} list (length {len(w)})"


def check_stats(ctx, cs, K, reps=1, port_stats=False):
    want = vp.add_counters(*[c.cnt for c in cs])
    got = ctx.counters()
    assert got == {k: reps * v for k, v in want.items()}, (got, want, reps)
    if port_stats:
        ps = ctx.port_stats()
        want = reps * sum(vp.port_stats(c.cl, c.ports, K) for c in cs)
        got = np.array([[ps[q]["rx_packets"], ps[q]["tx_packets"]] for q in range(K)])
        assert np.array_equal(got, want), (got, want)
        assert all(ps[q]["nf_dropped"] == ps[q]["rx_packets"] - ps[q]["tx_packets"] for q in range(K))


def run_submit(ctx, cs, mode, K=5, mis=0, port_stats=False):
    """All cases as batches of cop_submit launches (32 per launch)."""
    for lo in range(0, len(cs), 32):
        part = cs[lo:lo + 32]
        dp = ctx.alloc(sum(c.pk.nbytes for c in part))
        at, pos = [], 0
        for c in part:
            dp.upload(c.pk, pos)
            at.append(pos)
            pos += c.pk.nbytes
        rec = Guarded.packed(ctx, [c.n * 8 for c in part])
        cnt = Guarded.packed(ctx, [count_words(c.n, mode, K) * 4 for c in part], align=4)
        # every list `mis` words past a 16-byte boundary
        lst = Guarded.packed(ctx, [list_words(c.n, mode, K) * 4 for c in part], shift=4 * mis)
        for g in (rec, lst, cnt):
            g.fill()
        ctx.counters(reset=True)
        if port_stats:
            ctx.port_stats(reset=True)
        ctx.submit([cg.make_batch(dp, c.n, rec.addr(b), pkts_offset=at[b], fwd_idx=lst.addr(b), fwd_count=cnt.addr(b))
                    for b, c in enumerate(part)])
        ctx.sync()
        r, l, k = rec.read("records"), lst.read("lists"), cnt.read("counts")
        for b, c in enumerate(part):
            check_case(c, mode, K, r[b], l[b], k[b])
        check_stats(ctx, part, K, port_stats=port_stats)
        for x in (dp, rec.buf, lst.buf, cnt.buf):
            x.free()


def both_shapes(T, **kw):
    return cases(vp.ragged(T), T, **kw) + cases(3 * T, T, vp.WHOLE, **kw)


# ---------------------------------------------------------------------------
# one-shot kernel

@pytest.mark.parametrize("ppt", [1, 4, 8])
def test_oneshot_dense_lists(gpu_ctx_factory, monkeypatch, ppt):
    """compact_tile's single-list form staged in LDS, look_back over the
    batch's tiles, copy_out_list, flush_counters; every pattern at
    n = 3 T + 259 and a few at n = 3 T."""
    knobs(monkeypatch, COP_PPT=ppt)
    ctx = make_ctx(gpu_ctx_factory)
    run_submit(ctx, both_shapes(256 * ppt), "dense")


def test_oneshot_dense_lists_ticket_order(gpu_ctx_factory, monkeypatch):
    """The same with tiles drawn from tickets ($COP_STATIC_ORDER=0), which
    small launches otherwise never take."""
    knobs(monkeypatch, COP_PPT=4, COP_STATIC_ORDER=0)
    ctx = make_ctx(gpu_ctx_factory)
    run_submit(ctx, both_shapes(1024), "dense")


def test_oneshot_dense_lists_unstaged(gpu_ctx_factory, monkeypatch):
    """$COP_STAGE_LISTS=0: compact_tile's word stores straight from the lanes."""
    knobs(monkeypatch, COP_PPT=4, COP_STAGE_LISTS=0)
    ctx = make_ctx(gpu_ctx_factory)
    run_submit(ctx, both_shapes(1024), "dense")


@pytest.mark.parametrize("mis", [1, 2, 3])
def test_oneshot_dense_lists_misaligned(gpu_ctx_factory, monkeypatch, mis):
    """Every batch's fwd_idx 1, 2 or 3 words past a 16-byte boundary:
    copy_out_list's unaligned head and tail words."""
    knobs(monkeypatch, COP_PPT=4)
    ctx = make_ctx(gpu_ctx_factory)
    run_submit(ctx, cases(vp.ragged(1024), 1024), "dense", mis=mis)


@pytest.mark.parametrize("ppt", [1, 4, 8])
def test_oneshot_seg_lists(gpu_ctx_factory, monkeypatch, ppt):
    """COP_CFG_SEG_LISTS: seg_epilogue (segment lists staged in LDS, 16-byte
    chunks with the last clamped to n, counters_add)."""
    knobs(monkeypatch, COP_PPT=ppt)
    ctx = make_ctx(gpu_ctx_factory, flags=cg.CFG_SEG_LISTS)
    run_submit(ctx, both_shapes(256 * ppt), "seg")


def test_oneshot_seg_lists_port_stats(gpu_ctx_factory, monkeypatch):
    """SEG_LISTS | PORT_STATS: the EXT kernel, compact_tile's segmented form,
    flush_counters with the per-port statistics."""
    knobs(monkeypatch, COP_PPT=4)
    ctx = make_ctx(gpu_ctx_factory, flags=cg.CFG_SEG_LISTS | cg.CFG_PORT_STATS)
    run_submit(ctx, both_shapes(1024), "seg", port_stats=True)


def demux_cases(n, T, K, mask_names=vp.DEMUX_MASKS):
    return [case(m, n, T, K=K, layout=lay) for lay in vp.port_layouts(n, T, K) for m in mask_names]


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8])
def test_oneshot_demux(gpu_ctx_factory, monkeypatch, K):
    """DEMUX_PORTS | PORT_STATS with K vports: K look-back chains per tile;
    all forwards on one port (the other chains all zero), i % K, by wave and
    by tile, each with four forward masks."""
    knobs(monkeypatch, COP_PPT=4)
    ctx = make_ctx(gpu_ctx_factory, K=K, flags=cg.CFG_DEMUX_PORTS | cg.CFG_PORT_STATS)
    run_submit(ctx, demux_cases(vp.ragged(1024), 1024, K), "demux", K=K, port_stats=True)


def test_oneshot_long_chain_dense(gpu_ctx_factory, monkeypatch):
    """258 tiles of 256 packets: a look-back that reads more than 256
    predecessors, among them 257 that publish aggregate 0."""
    knobs(monkeypatch, COP_PPT=1)
    ctx = make_ctx(gpu_ctx_factory)
    run_submit(ctx, cases(vp.LONG_N, 256, vp.LONG_CHAIN), "dense")


def test_oneshot_long_chain_demux(gpu_ctx_factory, monkeypatch):
    """The same chain length with eight chains per tile."""
    knobs(monkeypatch, COP_PPT=1)
    K = 8
    ctx = make_ctx(gpu_ctx_factory, K=K, flags=cg.CFG_DEMUX_PORTS | cg.CFG_PORT_STATS)
    run_submit(ctx, demux_cases(vp.LONG_N, 256, K, ("all", "alt_tile_inv")), "demux", K=K, port_stats=True)


@pytest.mark.parametrize("flags,mode", [(0, "dense"), (cg.CFG_SEG_LISTS, "seg")])
def test_oneshot_route_hits(gpu_ctx_factory, monkeypatch, flags, mode):
    """Stages S | F | L with the route table in LDS: ROUTE_HIT prescribed as
    a mask independent of the verdicts, the route_hit counter and route_nh."""
    knobs(monkeypatch, COP_PPT=4)
    ctx = make_ctx(gpu_ctx_factory, flags=flags, stages=S | F | L)
    cs = cases(vp.ragged(1024), 1024, vp.ROUTE_CASES, lpm=True)
    assert any(0 < c.cnt["route_hit"] < c.cnt["pkt_total"] for c in cs)
    run_submit(ctx, cs, mode)


# ---------------------------------------------------------------------------
# poll-mode kernel

def pmd_knobs(monkeypatch, T):
    """256-packet tiles: six workers fit on a CU and fill it, and a host copy
    or memset beside the kernel then waits for its idle exit (a second).
    Four per CU ($COP_PMD_PER_CU) leave room, as the 1024-packet kernel's
    five do, so the ring wraps within one launch."""
    knobs(monkeypatch, COP_PPT=T // 256, **({"COP_PMD_PER_CU": 4} if T == 256 else {}))


class PatternRing:
    """A batch ring whose slots hold the given cases, outputs guarded."""

    def __init__(self, ctx, cs, mode, K=5):
        self.cs, self.mode, self.K = list(cs), mode, K
        P, n = len(cs), cs[0].n
        assert all(c.n == n for c in cs)
        self.dp = ctx.alloc(P * n * 64)
        for s, c in enumerate(cs):
            self.put(s, c)
        rslot = n + 8 + (n & 1)                  # even: the records go out as 16-byte stores from lane pairs
        words = list_words(n, mode, K)
        fslot = (words + 3) // 4 * 4 + 16
        cw = count_words(n, mode, K)
        self.rec = Guarded.strided(ctx, P, n * 8, rslot * 8)
        self.lst = Guarded.strided(ctx, P, words * 4, fslot * 4)
        self.cnt = Guarded.strided(ctx, P, cw * 4, cw * 4)     # counts are contiguous: guards at the two ends
        self.ring = cg.make_ring(self.dp, P, n, self.rec.addr(), n * 64, results_slot=rslot,
                                 fwd_idx=self.lst.addr(), fwd_slot=fslot, fwd_count=self.cnt.addr())

    def put(self, s, c):
        self.cs[s] = c
        self.dp.upload(c.pk, s * c.n * 64)

    def fill(self):
        for g in (self.rec, self.lst, self.cnt):
            g.fill()

    def check(self):
        r, l, k = self.rec.read("records"), self.lst.read("lists"), self.cnt.read("counts")
        for s, c in enumerate(self.cs):
            check_case(c, self.mode, self.K, r[s], l[s], k[s])


PMD_SEG = [(1024, 0, "cop_pmd<1, 0, 2, 4, false>"), (1024, cg.PMD_DYNAMIC_TILES, "cop_pmd<1, 0, 2, 4, false>"),
           (256, 0, "cop_pmd<1, 0, 2, 1, false>")]


@pytest.mark.parametrize("T,pflags,kname", PMD_SEG)
def test_pmd_seg_step_path(gpu_ctx_factory, monkeypatch, T, pflags, kname):
    """The step path (cop_tile.h tile_steps_v, emit / flush): at 1024-packet
    tiles a wave owns a segment and builds its list from a running count
    over four steps (static and dynamic tile order), at 256-packet tiles the
    barrier form with counters_add. Every pattern a ring slot, every slot
    posted twice with the outputs cleared in between."""
    pmd_knobs(monkeypatch, T)
    ctx = make_ctx(gpu_ctx_factory, flags=cg.CFG_SEG_LISTS)
    rg = PatternRing(ctx, cases(vp.ragged(T), T), "seg")
    P = len(rg.cs)
    ctx.counters(reset=True)
    with ctx.pmd_start(rg.ring, pflags) as m:
        assert m.info()["kernel_name"] == kname, m.info()
        for lap in range(2):
            rg.fill()
            m.post(P)
            m.wait()
            rg.check()
        assert m.info()["completed"] == 2 * P and m.info()["launches"] == 1
    check_stats(ctx, rg.cs, 5, reps=2)


LAPS = [("all", "first_tile_only"), ("none", "last_tile_only"), ("odd", "alt_tile"), ("even", "alt_tile_inv"),
        ("one_fwd@0", "tile_head_k"), ("one_drop@0", "bern_1_64")]


@pytest.mark.parametrize("T,kname", [(1024, "cop_pmd<1, 0, 2, 4, false>"), (256, "cop_pmd<1, 0, 2, 1, false>")])
def test_pmd_dense_chains_never_mix_across_laps(gpu_ctx_factory, monkeypatch, T, kname):
    """Dense lists on the poll-mode kernel (tile_body; the look-back chain's
    granules tagged with the batch sequence): a ring of two slots, rewritten
    with the inverse (or another) pattern before each lap and posted again.
    Each lap's lists and counts must be that lap's own: a chain never takes a
    granule its slot's previous batch published."""
    pmd_knobs(monkeypatch, T)
    ctx = make_ctx(gpu_ctx_factory)
    n = vp.ragged(T)
    rg = PatternRing(ctx, [case(x, n, T) for x in LAPS[0]], "dense")
    done = []
    ctx.counters(reset=True)
    with ctx.pmd_start(rg.ring) as m:
        assert m.info()["kernel_name"] == kname, m.info()
        for names in LAPS:
            for s, x in enumerate(names):
                rg.put(s, case(x, n, T))
            rg.fill()
            m.post(2)
            m.wait()
            rg.check()
            done += rg.cs
        assert m.info()["launches"] == 1
    check_stats(ctx, done, 5)


@pytest.mark.parametrize("K", [5, 8])
def test_pmd_demux(gpu_ctx_factory, monkeypatch, K):
    """The EXT poll-mode kernel with K look-back chains per tile."""
    knobs(monkeypatch, COP_PPT=4)
    ctx = make_ctx(gpu_ctx_factory, K=K, flags=cg.CFG_DEMUX_PORTS)
    rg = PatternRing(ctx, demux_cases(vp.ragged(1024), 1024, K), "demux", K=K)
    P = len(rg.cs)
    ctx.counters(reset=True)
    with ctx.pmd_start(rg.ring) as m:
        assert m.info()["kernel_name"] == "cop_pmd<1, 0, 2, 4, true>", m.info()
        for lap in range(2):
            rg.fill()
            m.post(P)
            m.wait()
            rg.check()
    check_stats(ctx, rg.cs, K, reps=2)


def test_pmd_seg_rule_counters(gpu_ctx_factory, monkeypatch):
    """SEG_LISTS | RULE_COUNTERS on the EXT poll-mode kernel: per-rule hits
    against the hit counts the prescription gives each rule."""
    knobs(monkeypatch, COP_PPT=4)
    ctx = make_ctx(gpu_ctx_factory, flags=cg.CFG_SEG_LISTS | cg.CFG_RULE_COUNTERS)
    rg = PatternRing(ctx, cases(vp.ragged(1024), 1024), "seg")
    P = len(rg.cs)
    ctx.counters(reset=True)
    ctx.rule_counters(reset=True)
    with ctx.pmd_start(rg.ring) as m:
        assert m.info()["kernel_name"] == "cop_pmd<1, 0, 2, 4, true>", m.info()
        rg.fill()
        m.post(P)
        m.wait()
        rg.check()
    check_stats(ctx, rg.cs, 5)
    want = sum(vp.rule_hits(c.cl) for c in rg.cs)
    assert want.min() > 0
    assert np.array_equal(ctx.rule_counters(), want)
