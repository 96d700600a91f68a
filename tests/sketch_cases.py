"""Inputs and expectations the sketch tests share (test_sketch_host.py on the
host, test_gpu_sketch.py on the device).

`Spec` restates the specification in include/cop_gpu.h ("Sketch") in numpy:
the hash, the counting rule, the estimate, and the police per list form. An
SkCase holds one batch in plain numpy: frames (or 16-byte records) whose every
byte is random except the fields set on purpose, verdict records, forward
lists in one of the three list forms (tx_cases.lay_lists), and the police
outputs (out_idx, out_count, status) between 0xAB guards. The same case runs
over host memory (cop_sketch_*_host) or is uploaded into one device buffer
(Pack) whose whole image is compared afterwards.
"""
import numpy as np

import copgpu as cg
import tx_cases as tc
import verdict_patterns as vp

GUARD, PAD, SEG = tc.GUARD, tc.PAD, cg.SEG_PKTS
M64 = (1 << 64) - 1
U64_MAX = M64
NS = (0, 1, 63, 64, 65, 255, 256, 257, 1027)
KINDS = ("one", "distinct", "heavy4", "same24", "mixed")
# name -> (stride, data_off); stride 0: IMIX offsets; stride 16: COP_HDR16_STRIDE records
LAYOUTS = {"s64": (64, 0), "s128": (128, 0), "s2176": (2176, 128), "imix": (0, 16), "rec16": (16, 0)}
VERDICT_MASKS = (0, 1, 2, 4, 8, 16)


def splitmix64(seed: int, count: int) -> list:
    out, s = [], seed & M64
    for _ in range(count):
        s = (s + 0x9E3779B97F4A7C15) & M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        out.append(z ^ (z >> 31))
    return out


class Spec:
    """The specification of one sketch configuration."""

    def __init__(self, rows=4, log2_cols=10, key=cg.SKETCH_KEY_SRC, key_depth=32, seed=0):
        self.rows, self.log2_cols, self.key, self.key_depth, self.seed = rows, log2_cols, key, key_depth, seed
        z = splitmix64(seed, rows)
        self.a = np.array([(x & 0xFFFFFFFF) | 1 for x in z], dtype=np.uint64)
        self.b = np.array([x >> 32 for x in z], dtype=np.uint64)
        self.cols = 1 << log2_cols

    def cfg(self) -> cg.SketchConfig:
        return cg.sketch_config(self.rows, self.log2_cols, self.key, self.key_depth, self.seed)

    def zeros(self) -> np.ndarray:
        return np.zeros((self.rows, self.cols), dtype=np.uint64)

    def key_of(self, addr) -> np.ndarray:
        return np.asarray(addr, dtype=np.uint64) >> np.uint64(32 - self.key_depth)

    def col(self, k) -> np.ndarray:
        """rows x len(k) columns."""
        k = np.asarray(k, dtype=np.uint64)
        return ((k[None, :] * self.a[:, None] + self.b[:, None]) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - self.log2_cols)

    def add(self, counters, keys):
        c = self.col(keys).astype(np.int64)
        for r in range(self.rows):
            np.add.at(counters[r], c[r], np.uint64(1))

    def est(self, counters, keys) -> np.ndarray:
        c = self.col(keys).astype(np.int64)
        return np.min(np.stack([counters[r][c[r]] for r in range(self.rows)]), axis=0) if len(c[0]) else \
            np.zeros(0, dtype=np.uint64)


def fields(pk: np.ndarray, starts: np.ndarray, rec: bool):
    """(counts as IPv4, src, dst) of the packets that start at `starts`."""
    eo, ao = (0, 6) if rec else (12, 26)
    s = starts.astype(np.int64)
    be = lambda o: sum(pk[s + o + j].astype(np.uint64) << np.uint64(24 - 8 * j) for j in range(4))
    ipv4 = (pk[s + eo] == 0x08) & (pk[s + eo + 1] == 0x00) & ((pk[s + eo + 2] >> 4) == 4)
    return ipv4, be(ao), be(ao + 4)


def addresses(kind: str, n: int, seed: int = 0) -> np.ndarray:
    """The traffic kinds: n addresses (u32 values in u64)."""
    rng = np.random.default_rng(0x5C0000 + seed)
    i = np.arange(n, dtype=np.uint64)
    light = np.uint64(0x0B000000) + (i * np.uint64(7919)) % np.uint64(1 << 24)
    heavy = np.array([0x0A010203, 0xC0A80001, 0xFFFFFFFF, 0x00000000], dtype=np.uint64)
    if kind == "one":
        return np.full(n, 0x0A010203 + seed, dtype=np.uint64)
    if kind == "distinct":
        return light
    if kind in ("heavy4", "mixed"):
        return np.where(rng.random(n) < 0.5, heavy[rng.integers(0, 4, n)], light)
    assert kind == "same24"
    return np.uint64(0xC0A80100) + i % np.uint64(251)


class SkCase:
    """One batch, its verdicts, its forward lists and the police outputs."""

    def __init__(self, n, kind="heavy4", layout="s64", form="dense", fwd=None, K=1, seed=0, threshold=0):
        self.n, self.kind, self.layout, self.form, self.K = n, kind, layout, form, K
        self.n_lists, self.seg = (K if form == "demux" else 1), form == "seg"
        stride, self.data_off = LAYOUTS[layout]
        self.rec, self.imix, self.stride = stride == 16, stride == 0, stride
        rng = np.random.default_rng(0x5CA5E + 131 * seed + n)
        m = max(n, 1)
        if self.imix:
            offsets = (rng.permutation(m) * 64).astype(np.uint32)
            pk = rng.integers(0, 256, m * 64 + 64, dtype=np.uint8)
            starts = offsets.astype(np.int64) + self.data_off
        else:
            pk = rng.integers(0, 256, m * stride + (self.data_off and 64), dtype=np.uint8)
            starts = np.arange(m, dtype=np.int64) * stride + self.data_off
        starts = starts[:n]
        src, dst = addresses(kind, n, seed), addresses(kind, n, seed + 7)[::-1]
        eo, ao = (0, 6) if self.rec else (12, 26)
        et = np.full(n, 0x0800)
        ver = np.full(n, 0x45)
        if kind == "mixed":
            u = rng.random(n)
            et[u < 1 / 8] = 0x86DD
            ver[(u >= 1 / 8) & (u < 1 / 8 + 1 / 16)] = 0x65
        pk[starts + eo], pk[starts + eo + 1], pk[starts + eo + 2] = et >> 8, et & 0xFF, ver
        for j in range(4):
            pk[starts + ao + j] = (src >> np.uint64(24 - 8 * j)) & np.uint64(0xFF)
            pk[starts + ao + 4 + j] = (dst >> np.uint64(24 - 8 * j)) & np.uint64(0xFF)
        res = np.zeros(m, dtype=cg.RESULT_DT)
        res["verdict"] = rng.integers(0, 5, m)
        res["flags"], res["port"], res["route_nh"] = rng.integers(0, 4, m), rng.integers(0, 8, m), rng.integers(0, 1 << 24, m)
        self.starts = starts
        self.inputs = {"pkts": pk, "results": res}
        if self.imix:
            self.inputs["offsets"] = offsets
        self.ipv4, self.src, self.dst = fields(pk, starts, self.rec)
        assert np.array_equal(self.src, src) and np.array_equal(self.dst, dst)
        self.verdict = res["verdict"][:n]
        # forward lists and the police outputs
        fwd = np.ones(n, dtype=bool) if fwd is None else fwd
        ports = (np.arange(n) // 7) % K
        idx, counts, _ = tc.lay_lists(form, n, fwd, ports, K)
        self.inputs["idx"], self.inputs["counts"] = idx, counts
        self.threshold = threshold
        words = lambda k: np.full((2 * PAD) // 4 + k, GUARD * 0x01010101, dtype=np.uint32)
        self.outs = [{"out_idx": words(len(idx)), "out_count": words(len(counts)), "status": words(4 * self.n_lists)}]
        self.expect = None

    # ---- the specification over this batch ----
    def counting(self, verdict_mask: int) -> np.ndarray:
        ok = self.ipv4.copy()
        if verdict_mask:
            ok &= ((verdict_mask >> self.verdict.astype(np.int64)) & 1).astype(bool)
        return ok

    def keys(self, spec: Spec) -> np.ndarray:
        return spec.key_of(self.dst if spec.key == cg.SKETCH_KEY_DST else self.src)

    def update(self, spec: Spec, counters, verdict_mask=0):
        spec.add(counters, self.keys(spec)[self.counting(verdict_mask)])

    def lists(self):
        """[(first word of the list in idx / out_idx, its entries as the clamps read them)]"""
        n, idx, cnt = self.n, self.inputs["idx"], self.inputs["counts"]
        if not n:
            return []
        if self.seg:
            return [(s * SEG, idx[s * SEG:s * SEG + min(int(cnt[s]), min(SEG, n - s * SEG))]) for s in range(len(cnt))]
        return [(q * n, idx[q * n:q * n + min(int(cnt[q]), n)]) for q in range(self.n_lists)]

    def police(self, spec: Spec, counters, threshold=None):
        """Sets self.expect: what the outputs must hold afterwards."""
        th = self.threshold if threshold is None else threshold
        e = {k: v.copy() for k, v in self.outs[0].items()}
        o, keys, st = PAD // 4, self.keys(spec), []
        for li, (first, ent) in enumerate(self.lists()):
            i = np.minimum(ent.astype(np.int64), self.n - 1)
            keep = ~self.ipv4[i] | (spec.est(counters, keys[i]) < np.uint64(th))
            kept = ent[keep]
            e["out_idx"][o + first:o + first + len(kept)] = kept
            e["out_count"][o + li] = len(kept)
            st.append((len(kept), len(ent) - len(kept)))
        if self.n:
            if self.seg:
                st = [tuple(np.sum(st, axis=0))]
            for q, (k, r) in enumerate(st):
                e["status"][o + 4 * q:o + 4 * q + 4] = (k, r, 0, 0)
        self.expect = [e]
        return e

    def median_threshold(self, spec: Spec, counters) -> int:
        ests = np.concatenate([spec.est(counters, self.keys(spec)[np.minimum(e.astype(np.int64), self.n - 1)])
                               for _, e in self.lists()] or [np.zeros(1, dtype=np.uint64)])
        return int(np.median(ests)) if len(ests) else 0

    # ---- descriptors ----
    def descs(self, addr_in, addr_out, with_results=True):
        """(Batch, PoliceDesc); addr_in(name) / addr_out(q, name) the base address of that array."""
        b = cg.Batch()
        if self.n:
            b.pkts, b.fwd_idx, b.fwd_count = addr_in("pkts"), addr_in("idx"), addr_in("counts")
            if with_results:
                b.results = addr_in("results")
        if self.imix:
            b.offsets = addr_in("offsets")
        b.n, b.stride, b.data_off = self.n, self.stride, self.data_off
        p = cg.PoliceDesc()
        p.threshold = self.threshold
        if self.n:
            p.out_idx, p.out_count, p.status = (addr_out(0, k) + PAD for k in ("out_idx", "out_count", "status"))
        return b, p

    def check(self, got_of):
        for k, want in self.expect[0].items():
            got = got_of(0, k)
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                raise AssertionError(f"{k} ({self.form}, n={self.n}, {self.layout}, {self.kind}): {len(bad)} words differ, "
                                     f"first at {bad[:6]} (guard {PAD // 4} words; got {got[bad[:6]]}, want {want[bad[:6]]})")


def host_descs(cases, with_results=True):
    """(batches, police descs, keep-alive) over the cases' own host arrays."""
    keep, bs, ps = [], [], []

    def hold(a):
        keep.append(a)
        return a.ctypes.data

    for c in cases:
        c.inputs["pkts"] = _aligned_copy(c.inputs["pkts"])
        for k in c.outs[0]:
            c.outs[0][k] = _aligned_copy(c.outs[0][k])
        b, p = c.descs(lambda name, c=c: hold(c.inputs[name]), lambda q, k, c=c: hold(c.outs[q][k]), with_results)
        bs.append(b)
        ps.append(p)
    return bs, ps, keep


def _aligned_copy(a: np.ndarray) -> np.ndarray:
    raw = tc.aligned(a.nbytes)
    raw[:] = a.view(np.uint8)
    return raw.view(a.dtype)


def true_counts(keys: np.ndarray) -> dict:
    u, c = np.unique(keys, return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


class Pack:
    """All arrays of some cases, and `extra` named arrays, in one device buffer, 256 bytes apart or more."""

    def __init__(self, ctx, cases, extra=None):
        self.cases, self.at, pos = cases, {}, 256
        items = [((ci, "in", 0, name), a) for ci, c in enumerate(cases) for name, a in c.inputs.items()]
        items += [((ci, "out", 0, k), a) for ci, c in enumerate(cases) for k, a in c.outs[0].items()]
        items += [((-1, "x", 0, name), a) for name, a in (extra or {}).items()]
        for key, a in items:
            self.at[key] = (pos, a)
            pos = (pos + a.nbytes + 511) & ~255
        self.img = np.full(pos, 0x5A, dtype=np.uint8)
        for o, a in self.at.values():
            self.img[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8)
        self.buf = ctx.alloc(pos)
        self.buf.upload(self.img)
        self.raw = None

    def addr(self, ci, kind, q, name):
        return self.buf.addr + self.at[(ci, kind, q, name)][0]

    def x(self, name):
        return self.addr(-1, "x", 0, name)

    def descs(self, with_results=True):
        out = [c.descs(lambda name, ci=ci: self.addr(ci, "in", 0, name), lambda q, k, ci=ci: self.addr(ci, "out", q, k),
                       with_results) for ci, c in enumerate(self.cases)]
        return [b for b, _ in out], [p for _, p in out]

    def got(self, ci, kind, q, name):
        o, a = self.at[(ci, kind, q, name)]
        return self.raw[o:o + a.nbytes].view(a.dtype)

    def download(self):
        self.raw = self.buf.download(np.uint8, self.buf.nbytes)

    def check(self, outputs=(), extra_want=None):
        """The whole image: only the police outputs named in `outputs` (case
        indices) and the extra arrays of extra_want may differ, and they hold
        what is expected."""
        self.download()
        want = self.img.copy()
        for ci in outputs:
            for k, e in self.cases[ci].expect[0].items():
                o, a = self.at[(ci, "out", 0, k)]
                want[o:o + a.nbytes] = e.view(np.uint8)
                self.cases[ci].check(lambda q, k, ci=ci: self.got(ci, "out", q, k))
        for name, a in (extra_want or {}).items():
            o, _ = self.at[(-1, "x", 0, name)]
            got = self.raw[o:o + a.nbytes].view(a.dtype)
            assert np.array_equal(got, a), (name, np.nonzero(got != a)[0][:6])
            want[o:o + a.nbytes] = a.view(np.uint8)
        bad = np.nonzero(self.raw != want)[0]
        assert bad.size == 0, f"bytes outside the outputs changed at {bad[:8]}"
