"""The overlap rules of the four side-call validators (cop_tx_validate,
cop_sketch_police_validate, cop_aead_validate, cop_fwd_check_validate /
cop_fwd_rewrite_validate), called through ctypes: which pairs of extents may
meet and which may not, and the reason each refusal gives.

The validators only compare addresses, so the extents here are address ranges
that nothing backs: every one 1 MiB from the next. Each case is an accepted
call at n = 257 with two batches (a slot batch and an IMIX batch, whose slab is
represented by its first 16 bytes). A written extent W is then moved against
every other extent X of the call, to the two least overlaps its alignment
allows:
  - W's last bytes over X's first (one byte where W's size is free: the
    frames of a burst are given 16 k + 1 bytes; else one alignment unit);
  - W's first aligned position inside X's last bytes;
and to the two nearest positions that only touch X, which are accepted.
W over a read extent is -EINVAL for every validator; W over another written
extent is accepted by tx and police (outputs may meet each other) and -EINVAL
for aead and fwd. No GPU.
"""
import ctypes
from ctypes import POINTER, byref, c_char_p, c_int, c_uint32, c_void_p

import pytest

import copgpu as cg

EINVAL = -22
N = 257
BASE = 1 << 32
GAP = 1 << 20
TX_WHY = b"an output extent overlaps a batch's packets, offsets, lens, records or lists"
POL_WHY = b"an output extent overlaps a batch's packets, offsets, records or lists, or the sketch's counters"
AEAD_WHY = b"frames, tags, ok or status overlaps another extent of the call"
FWD_WHY = b"an output extent overlaps another extent of the call or the table"
CAP_BYTES = N * 64 + 1


def _fn(name, *argtypes):
    f = getattr(ctypes.CDLL(cg.lib()._name), name)   # a handle of its own: the package's signatures stay as they are
    f.restype = c_int
    f.argtypes = list(argtypes) + [POINTER(c_char_p)]
    return f


class Call:
    """extents: name -> (bytes, alignment, written); run(addr) -> (rc, why)"""

    def __init__(self, extents, run):
        self.ext = extents
        self.base = {name: BASE + i * GAP for i, name in enumerate(extents)}
        self.run = run

    def written(self):
        return [k for k, (_, _, w) in self.ext.items() if w]

    def moved(self, w, x, how):
        size, align, _ = self.ext[w]
        xs, xe = self.base[x], self.base[x] + self.ext[x][0]
        at = {"tail_over_head": xs - (size - 1) // align * align,
              "head_over_tail": (xe - 1) // align * align,
              "ends_at": xs - -(-size // align) * align,
              "starts_at": -(-xe // align) * align}[how]
        if how == "tail_over_head":
            assert at <= xs < at + size <= xs + align
        if how == "head_over_tail":
            assert xs <= at < xe and xe - at <= align
        a = dict(self.base)
        a[w] = at
        return self.run(a)


def batches_of(a, seg, results=True):
    bs = (cg.Batch * 2)()
    for j, b in enumerate(bs):
        b.pkts, b.n, b.data_off = a[f"pkts{j}"], N, 0
        b.offsets, b.stride = (a["offsets1"], 0) if j else (None, 64)
        b.results = a[f"results{j}"] if results else None
        b.fwd_idx, b.fwd_count = a[f"fwd_idx{j}"], a[f"fwd_count{j}"]
    return bs


def batch_extents(seg, lens=True, results=True):
    words = (N + 255) // 256 if seg else 1
    e = {}
    for j in range(2):
        e[f"pkts{j}"] = (16 if j else N * 64, 16, False)
        if j:
            e["offsets1"] = (4 * N, 4, False)
            if lens:
                e["lens1"] = (4 * N, 4, False)
        if results:
            e[f"results{j}"] = (8 * N, 8, False)
        e[f"fwd_idx{j}"] = (4 * N, 4, False)
        e[f"fwd_count{j}"] = (4 * words, 4, False)
    return e, words


def tx_descs(a):
    tx = (cg.TxDesc * 2)()
    for j, t in enumerate(tx):
        t.lens = a["lens1"] if j else None
        t.copy_bytes = t.slot_bytes = 0 if j else 64
        o = t.out[0]
        o.frames, o.off, o.len, o.status = a[f"frames{j}"], a[f"off{j}"], a[f"len{j}"], a[f"tx_status{j}"]
        o.cap_bytes, o.cap_frames = CAP_BYTES, N
    return tx


def burst_extents(written_too):
    e = {}
    for j in range(2):
        e[f"frames{j}"] = (CAP_BYTES, 16, True)
        e[f"off{j}"] = (4 * N, 4, written_too)
        e[f"len{j}"] = (4 * N, 4, written_too)
        e[f"tx_status{j}"] = (16, 16, written_too)
    return e


def tx_call(seg):
    f = _fn("cop_tx_validate", POINTER(cg.Batch), POINTER(cg.TxDesc), c_uint32, c_uint32, c_int, c_uint32)
    e, _ = batch_extents(seg)
    e.update(burst_extents(True))

    def run(a):
        why = c_char_p()
        rc = f(batches_of(a, seg), tx_descs(a), 2, 1, int(seg), 0, byref(why))
        return rc, why.value
    return Call(e, run)


def police_call(seg):
    f = _fn("cop_sketch_police_validate", POINTER(cg.SketchConfig), c_void_p, POINTER(cg.Batch),
            POINTER(cg.PoliceDesc), c_uint32, c_uint32, c_int, c_uint32)
    cfg = cg.SketchConfig(rows=2, log2_cols=4, key=0, key_depth=32, seed=1)
    e, words = batch_extents(seg, lens=False)
    e["counters"] = (2 * 16 * 8, 8, False)
    for j in range(2):
        e[f"out_idx{j}"] = (4 * N, 4, True)
        e[f"out_count{j}"] = (4 * words, 4, True)
        e[f"status{j}"] = (16, 16, True)

    def run(a):
        pol = (cg.PoliceDesc * 2)()
        for j, p in enumerate(pol):
            p.threshold, p.out_idx, p.out_count, p.status = 5, a[f"out_idx{j}"], a[f"out_count{j}"], a[f"status{j}"]
        why = c_char_p()
        rc = f(byref(cfg), a["counters"], batches_of(a, seg), pol, 2, 1, int(seg), 0, byref(why))
        return rc, why.value
    return Call(e, run)


def aead_call(mode):
    f = _fn("cop_aead_validate", POINTER(cg.AeadKey), POINTER(cg.AeadBurst), c_uint32, c_int, c_void_p, c_uint32)
    key = cg.AeadKey()
    e = {}
    for j in range(2):
        e[f"frames{j}"] = (CAP_BYTES, 16, True)
        e[f"tags{j}"] = (16 * N, 16, True)
        if mode == 1:
            e[f"ok{j}"] = (4 * N, 4, True)
        e[f"status{j}"] = (16, 16, True)
        e[f"off{j}"] = (4 * N, 4, False)
        e[f"len{j}"] = (4 * N, 4, False)
        e[f"count{j}"] = (4, 4, False)
    if mode == 2:
        e["otk"] = (32 * N, 4, False)

    def run(a):
        bursts = (cg.AeadBurst * 2)()
        for j, b in enumerate(bursts):
            b.frames, b.off, b.len, b.count, b.tags = a[f"frames{j}"], a[f"off{j}"], a[f"len{j}"], a[f"count{j}"], a[f"tags{j}"]
            b.ok, b.status = a.get(f"ok{j}"), a[f"status{j}"]
            b.cap_bytes, b.seq_base, b.n_frames, b.aad_bytes = CAP_BYTES, 7, N, 8
        why = c_char_p()
        rc = f(byref(key), bursts, 2, mode, a.get("otk"), 0, byref(why))
        return rc, why.value
    return Call(e, run)


def fwd_check_call(seg):
    f = _fn("cop_fwd_check_validate", c_void_p, c_uint32, POINTER(cg.FwdConfig), POINTER(cg.Batch),
            POINTER(cg.FwdCheckDesc), c_uint32, c_uint32, c_int, c_uint32)
    cfg = cg.FwdConfig(flags=0, miss_nh=0)
    e, words = batch_extents(seg)
    e["entries"] = (16 * 8, 16, False)
    for j in range(2):
        e[f"out_idx{j}"] = (4 * N, 4, True)
        e[f"out_count{j}"] = (4 * words, 4, True)
        e[f"exc_idx{j}"] = (4 * N, 4, True)
        e[f"exc_count{j}"] = (4 * words, 4, True)
        e[f"status{j}"] = (16, 16, True)

    def run(a):
        desc = (cg.FwdCheckDesc * 2)()
        for j, d in enumerate(desc):
            d.lens = a["lens1"] if j else None
            d.out_idx, d.out_count, d.exc_idx, d.exc_count = a[f"out_idx{j}"], a[f"out_count{j}"], a[f"exc_idx{j}"], a[f"exc_count{j}"]
            d.status = a[f"status{j}"]
        why = c_char_p()
        rc = f(a["entries"], 8, byref(cfg), batches_of(a, seg), desc, 2, 1, int(seg), 0, byref(why))
        return rc, why.value
    return Call(e, run)


def fwd_rewrite_call(seg):
    f = _fn("cop_fwd_rewrite_validate", c_void_p, c_uint32, POINTER(cg.FwdConfig), POINTER(cg.Batch),
            POINTER(cg.TxDesc), POINTER(cg.FwdRwDesc), c_uint32, c_uint32, c_int, c_uint32)
    cfg = cg.FwdConfig(flags=0, miss_nh=0)
    e, _ = batch_extents(seg)
    e.update(burst_extents(False))   # the rewrite reads off, len and the gather's status
    e["entries"] = (16 * 8, 16, False)
    for j in range(2):
        e[f"port{j}"] = (4 * N, 4, True)
        e[f"status{j}"] = (16, 16, True)

    def run(a):
        rw = (cg.FwdRwDesc * 2)()
        for j, r in enumerate(rw):
            r.port[0], r.status[0] = a[f"port{j}"], a[f"status{j}"]
        why = c_char_p()
        rc = f(a["entries"], 8, byref(cfg), batches_of(a, seg), tx_descs(a), rw, 2, 1, int(seg), 0, byref(why))
        return rc, why.value
    return Call(e, run)


# the gather's own rule runs first inside cop_fwd_rewrite_validate: its outputs against what it reads
TX_OUT = ("frames", "off", "len", "tx_status")
TX_IN = ("pkts", "offsets", "lens", "results", "fwd_idx", "fwd_count")
# what the rewrite itself does not look at (the gather has read them already)
RW_UNSEEN = ("pkts", "offsets", "lens")


def kind(name):
    return name.rstrip("01")


def rewrite_expect(w, x, call):
    if kind(w) in TX_OUT and kind(x) in TX_IN:
        return EINVAL, TX_WHY
    if kind(x) in TX_OUT and kind(w) in TX_IN:   # never: w is written
        return EINVAL, TX_WHY
    if kind(x) in RW_UNSEEN:
        return 0, b""
    return EINVAL, FWD_WHY


CASES = {
    "tx": (tx_call, (False, True), lambda w, x, c: (0, b"") if c.ext[x][2] else (EINVAL, TX_WHY)),
    "police": (police_call, (False, True), lambda w, x, c: (0, b"") if c.ext[x][2] else (EINVAL, POL_WHY)),
    "aead": (aead_call, (0, 1, 2), lambda w, x, c: (EINVAL, AEAD_WHY)),
    "fwd_check": (fwd_check_call, (False, True), lambda w, x, c: (EINVAL, FWD_WHY)),
    "fwd_rewrite": (fwd_rewrite_call, (False, True), rewrite_expect),
}


@pytest.mark.parametrize("name,variant", [(k, v) for k, (_, vs, _) in CASES.items() for v in vs])
def test_which_extents_may_meet(name, variant):
    make, _, expect = CASES[name]
    call = make(variant)
    assert call.run(call.base) == (0, b"")
    pairs = 0
    for w in call.written():
        for x in call.ext:
            if x == w:
                continue
            want = expect(w, x, call)
            for how in ("tail_over_head", "head_over_tail"):
                assert call.moved(w, x, how) == want, (w, x, how)
            for how in ("ends_at", "starts_at"):
                assert call.moved(w, x, how) == (0, b""), (w, x, how)
            pairs += 1
    assert pairs >= 2 * len(call.written())
