"""Inputs and expectations the tx-gather tests share (test_tx_gather_host.py on
the host, test_gpu_tx_gather.py on the device).

A TxCase holds one batch in plain numpy: the packets (random bytes, so a
misplaced 16-byte piece shows), the forward lists laid out in one of the three
list forms, and per list a tx burst whose every extent (frames, off, len,
status) sits between 0xAB guards. `expect` is what the extents must hold
afterwards, guards, gaps and unwritten tails included, from `restate`, a
numpy restatement of the semantics in include/cop_gpu.h. The same case runs
over host memory (cop_tx_gather_host) or is uploaded to device buffers.
"""
import numpy as np

import copgpu as cg
import verdict_patterns as vp

GUARD = 0xAB
PAD = 64                       # guard bytes on each side of every output extent (keeps 16-byte alignment)
SEG = cg.SEG_PKTS
JUNK = 0xDEADBEEF              # list words no count covers: never read
IMIX_LENS = (1, 15, 16, 17, 60, 64, 594, 1518, 2048)


def restate(L, n, lens, copy_bytes, slot_bytes, cap_bytes, cap_frames):
    """(W, off[:W], len[:W], ext[:W], status) of list L."""
    L = np.minimum(np.asarray(L, dtype=np.int64), n - 1)
    k = np.arange(len(L), dtype=np.int64)
    if lens is None:
        ln = ext = np.full(len(L), copy_bytes, dtype=np.int64)
        off = k * slot_bytes
    else:
        ln = np.clip(lens[L].astype(np.int64), 1, cg.TX_MAX_FRAME)
        ext = (ln + 15) & ~15
        off = np.cumsum(ext) - ext
    ok = (k < cap_frames) & (off + ext <= cap_bytes)
    W = int(ok.sum())
    assert ok[:W].all()                                   # monotone: the written frames are a prefix
    used = int(off[W - 1] + ext[W - 1]) if W else 0
    return W, off[:W], ln[:W], ext[:W], np.array([W, used, len(L) - W, 0], dtype=np.uint32)


def aligned(nbytes: int, fill: int = 0) -> np.ndarray:
    """A u8 array of nbytes whose first byte is 64-byte aligned."""
    raw = np.full(nbytes + 64, fill, dtype=np.uint8)
    o = (-raw.ctypes.data) % 64
    return raw[o:o + nbytes]


def lay_lists(form: str, n: int, fwd, ports=None, K: int = 1):
    """(fwd_idx words, fwd_count words, the list of every burst) of a forward
    mask in a list form: "dense", "seg" or "demux" (K vports)."""
    if form == "dense":
        L = vp.dense_list(fwd)
        idx = np.full(max(n, 1), JUNK, dtype=np.uint32)
        idx[:len(L)] = L
        return idx, np.array([len(L)], dtype=np.uint32), [L]
    if form == "seg":
        counts, lists = vp.seg_lists(fwd) if n else (np.zeros(0, np.uint32), [])
        idx = np.full(max(n, 1), JUNK, dtype=np.uint32)
        for s, l in enumerate(lists):
            idx[s * SEG:s * SEG + len(l)] = l
        whole = np.concatenate(lists) if lists else np.zeros(0, np.uint32)
        return idx, (counts if n else np.zeros(1, np.uint32)), [whole]
    assert form == "demux"
    counts, lists = vp.port_lists(fwd, ports, K)
    idx = np.full(max(K * n, 1), JUNK, dtype=np.uint32)
    for q, l in enumerate(lists):
        idx[q * n:q * n + len(l)] = l
    return idx, counts, lists


class TxCase:
    """One batch and its bursts. Source: slot (stride, data_off, copy_bytes,
    slot_bytes) or IMIX (offsets, lens). caps: per burst (cap_bytes,
    cap_frames) or None for room for everything plus a spare frame."""

    def __init__(self, pk, n, form, idx, counts, lists, stride=64, data_off=0, copy_bytes=0, slot_bytes=0,
                 offsets=None, lens=None, caps=None, no_off_len=False):
        self.n, self.form, self.lists = n, form, lists
        self.n_lists, self.seg = (len(lists) if form == "demux" else 1), form == "seg"
        self.stride, self.data_off = stride, data_off
        self.copy_bytes, self.slot_bytes = copy_bytes, (slot_bytes or copy_bytes)
        self.imix = offsets is not None
        self.inputs = {"pkts": pk, "idx": idx, "counts": counts}
        if self.imix:
            self.inputs["offsets"] = np.asarray(offsets, dtype=np.uint32)
            self.inputs["lens"] = np.asarray(lens, dtype=np.uint32)
            self.stride = self.copy_bytes = self.slot_bytes = 0
        self.outs, self.expect, self.caps = [], [], []
        start = (self.inputs["offsets"].astype(np.int64) if self.imix else np.arange(n, dtype=np.int64) * stride) + data_off
        for q, L in enumerate(lists):
            if caps is not None and caps[q] is not None:
                cap_bytes, cap_frames = caps[q]
            else:
                _, off, _, ext, st = restate(L, n, self.inputs.get("lens"), self.copy_bytes, self.slot_bytes, 1 << 40, 1 << 40)
                cap_bytes, cap_frames = int(st[1]) + 48, len(L) + 3
            W, off, ln, ext, st = restate(L, n, self.inputs.get("lens"), self.copy_bytes, self.slot_bytes, cap_bytes, cap_frames)
            self.caps.append((cap_bytes, cap_frames))
            fr = np.full(PAD + cap_bytes + PAD, GUARD, dtype=np.uint8)
            words = lambda m: np.full((PAD + 4 * m + PAD) // 4, GUARD * 0x01010101, dtype=np.uint32)
            o = {"frames": fr, "off": words(cap_frames), "len": words(cap_frames), "status": words(4)}
            if no_off_len:
                del o["off"], o["len"]
            e = {k: v.copy() for k, v in o.items()}
            Lc = np.minimum(np.asarray(L, dtype=np.int64), max(n - 1, 0))
            for k in range(W):
                s = int(start[Lc[k]])
                e["frames"][PAD + int(off[k]):PAD + int(off[k] + ext[k])] = pk[s:s + int(ext[k])]
            if not no_off_len:
                e["off"][PAD // 4:PAD // 4 + W] = off
                e["len"][PAD // 4:PAD // 4 + W] = ln
            e["status"][PAD // 4:PAD // 4 + 4] = st
            self.outs.append(o)
            self.expect.append(e)

    def descs(self, addr_in, addr_out):
        """(Batch, TxDesc) with addr_in(name) / addr_out(q, name) the base
        address of that array (outputs: of its guard; None if absent)."""
        b = cg.Batch()
        if self.n:
            b.pkts = addr_in("pkts")
            b.fwd_idx, b.fwd_count = addr_in("idx"), addr_in("counts")
        if self.imix:
            b.offsets = addr_in("offsets")   # an empty IMIX batch is still IMIX
        b.n, b.stride, b.data_off = self.n, self.stride, self.data_off
        t = cg.TxDesc()
        if self.imix and self.n:
            t.lens = addr_in("lens")
        t.copy_bytes, t.slot_bytes = self.copy_bytes, self.slot_bytes
        for q in range(len(self.lists)):
            o = t.out[q]
            for k in ("frames", "off", "len", "status"):
                a = addr_out(q, k)
                setattr(o, k, None if a is None else a + PAD)
            o.cap_bytes, o.cap_frames = self.caps[q]
        return b, t

    def check(self, got_of):
        """got_of(q, name) -> the array as it is now."""
        for q, e in enumerate(self.expect):
            for k, want in e.items():
                got = got_of(q, k)
                if not np.array_equal(got, want):
                    bad = np.nonzero(got != want)[0]
                    raise AssertionError(f"burst {q} {k}: {len(bad)} differ, first at {bad[:6]} "
                                         f"(guard {PAD} bytes; got {got[bad[:6]]}, want {want[bad[:6]]}); "
                                         f"status got {got_of(q, 'status')[PAD // 4:PAD // 4 + 4]} "
                                         f"want {e['status'][PAD // 4:PAD // 4 + 4]}")


def slot_packets(n: int, stride: int, seed: int = 1) -> np.ndarray:
    return np.random.default_rng(0x7C0000 + seed).integers(0, 256, max(n, 1) * stride, dtype=np.uint8)


def slot_case(n, form, fwd, stride=64, data_off=0, copy_bytes=64, slot_bytes=0, ports=None, K=1, caps=None, pk=None,
              no_off_len=False) -> TxCase:
    idx, counts, lists = lay_lists(form, n, fwd, ports, K)
    pk = slot_packets(n, stride) if pk is None else pk
    return TxCase(pk, n, form, idx, counts, lists, stride=stride, data_off=data_off, copy_bytes=copy_bytes,
                  slot_bytes=slot_bytes, caps=caps, no_off_len=no_off_len)


def imix_source(n: int, lens_cycle=IMIX_LENS, seed: int = 2):
    """(slab, offsets, lens): offsets at 64-byte steps in a shuffled order,
    lens cycling; the slab ends COP_TX_MAX_FRAME + 16 readable bytes past the last offset."""
    rng = np.random.default_rng(0x7C1000 + seed)
    offsets = (rng.permutation(max(n, 1)) * 64).astype(np.uint32)
    lens = np.array([lens_cycle[i % len(lens_cycle)] for i in range(max(n, 1))], dtype=np.uint32)
    slab = rng.integers(0, 256, max(n, 1) * 64 + cg.TX_MAX_FRAME + 64, dtype=np.uint8)
    return slab, offsets, lens


def imix_case(n, form, fwd, lens_cycle=IMIX_LENS, data_off=0, ports=None, K=1, caps=None, no_off_len=False,
              lens=None) -> TxCase:
    idx, counts, lists = lay_lists(form, n, fwd, ports, K)
    slab, offsets, ln = imix_source(n, lens_cycle)
    return TxCase(slab, n, form, idx, counts, lists, data_off=data_off, offsets=offsets,
                  lens=ln if lens is None else lens, caps=caps, no_off_len=no_off_len)


def masks(n: int) -> dict:
    """The forward masks the tests run at n packets (verdict_patterns.patterns names)."""
    if n == 0:
        return {"none": np.zeros(0, dtype=bool)}
    p = vp.patterns(n, 256)
    names = ["none", "all", "alt_wave", "alt_seg", "seg_head_k", "seg_tail_k", "bern_1_64", "bern_63_64"]
    names += [k for k in p if k.startswith(("one_fwd@", "one_drop@"))]
    return {k: p[k] for k in names}


def cap_cases(case_of):
    """The capacity cases of one list: case_of(caps) builds the case; yields
    (name, case). |L| must be > 300 so that a cut falls into the second chunk."""
    full = case_of(None)
    L = full.lists[0]
    W, off, ln, ext, st = restate(L, full.n, full.inputs.get("lens"), full.copy_bytes, full.slot_bytes, 1 << 40, 1 << 40)
    assert W == len(L) > 300
    room = int(st[1]) + 64
    for cf in (0, 1, len(L) - 1, len(L)):
        yield f"cap_frames={cf}", case_of([(room, cf)])
    end = int(off[200] + ext[200])
    mid = int(off[300] + ext[300]) - 16       # in the middle of the second chunk, inside a frame
    for name, cb in (("at_frame_end", end), ("one_byte_short", end - 1), ("mid_chunk2", mid), ("zero", 0),
                     ("exact", int(st[1])), ("chunk_boundary", int(off[255] + ext[255]))):
        yield f"cap_bytes:{name}", case_of([(cb, len(L) + 5)])


def run_host(cases, max_batch: int = 0) -> int:
    """cop_tx_gather_host over the cases' own arrays (one call); returns its code."""
    keep = []

    def hold(a):
        keep.append(a)
        return a.ctypes.data

    bs, ts = [], []
    for c in cases:
        b, t = c.descs(lambda name: hold(c.inputs[name]), lambda q, k: hold(c.outs[q][k]) if k in c.outs[q] else None)
        bs.append(b)
        ts.append(t)
    return cg.tx_gather_host(bs, ts, cases[0].n_lists, cases[0].seg, max_batch)


def host_arrays_aligned(c: TxCase):
    """Move the case's packets and outputs into 64-byte aligned host arrays."""
    a = aligned(c.inputs["pkts"].nbytes)
    a[:] = c.inputs["pkts"]
    c.inputs["pkts"] = a
    for o in c.outs:
        for k in list(o):
            raw = aligned(o[k].nbytes)
            raw[:] = o[k].view(np.uint8)
            o[k] = raw.view(o[k].dtype)
    return c
