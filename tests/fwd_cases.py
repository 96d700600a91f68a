"""Inputs and expectations the L3-forward tests share (test_fwd_host.py on the
host, test_gpu_fwd.py on the device).

This module restates the specification in include/cop_gpu.h ("L3 forward") in
numpy: the classes (`classify`), the rewrite with the RFC 1624 checksum update
(`rewrite_rows`), the check per list form and the rewrite per burst. An
FwdCase holds one batch in plain numpy, built like sketch_cases.SkCase: frames
whose every byte is random except the fields set on purpose, verdict records,
forward lists in one of the three list forms, and every output between 0xAB
guards. The class of packet i is prescribed, PATTERN[i % len(PATTERN)], and
its header and record are constructed to land in it, so every class occurs in
every case with n >= 63. The same case runs over host memory or is uploaded
into one device buffer (sketch_cases.Pack) whose whole image is compared
afterwards.
"""
import numpy as np

import copgpu as cg
import sketch_cases as sc
import tx_cases as tc

GUARD, PAD, SEG = tc.GUARD, tc.PAD, cg.SEG_PKTS
OK, PASS, SHORT, BAD_HDR, OPTIONS, BAD_CSUM, TTL, NO_NEIGH = (cg.FWD_OK, cg.FWD_PASS, cg.FWD_SHORT, cg.FWD_BAD_HDR,
                                                              cg.FWD_OPTIONS, cg.FWD_BAD_CSUM, cg.FWD_TTL,
                                                              cg.FWD_NO_NEIGH)
PATTERN = (OK, PASS, OK, TTL, OK, NO_NEIGH, SHORT, OK, BAD_HDR, OPTIONS, OK, BAD_CSUM, PASS)
# name -> (stride, data_off, copy_bytes, slot_bytes); stride 0: IMIX offsets
LAYOUTS = {"s64": (64, 0, 64, 64), "s128": (128, 0, 112, 128), "s2176": (2176, 128, 48, 64), "imix": (0, 16, 0, 0)}
SHORT_LENS = (0, 1, 20, 33)
LONG_LENS = (34, 48, 60, 64, 594, 1518, 5000)
MISS = ("valid", "invalid", "none")


def fold(v):
    v = np.asarray(v, dtype=np.int64)
    for _ in range(3):
        v = (v & 0xFFFF) + (v >> 16)
    return v


def words_be(h, lo, cnt):
    """cnt big-endian 16-bit words of the rows of h from byte lo."""
    w = h[:, lo:lo + 2 * cnt].astype(np.int64).reshape(len(h), cnt, 2)
    return (w[:, :, 0] << 8) | w[:, :, 1]


def csum_full(h):
    """The IPv4 header checksum of rows of frames (bytes 14..33), recomputed with bytes 24..25 as zero."""
    w = words_be(h, 14, 10)
    w[:, 5] = 0
    return ~fold(w.sum(axis=1)) & 0xFFFF


def classify(h, short, res, tab, n_entries, flags, miss_nh):
    """The class of every row of h (34 frame bytes each), lowest priority first so the first match wins."""
    m = len(h)
    cls = np.full(m, OK, dtype=np.int64)
    hit = (res["flags"] & cg.FLAG_ROUTE_HIT).astype(bool) if res is not None else np.zeros(m, dtype=bool)
    nh = np.where(hit, res["route_nh"].astype(np.int64) & 0xFFFFFF, miss_nh) if res is not None else np.full(m, miss_nh)
    inr = nh < n_entries
    valid = np.zeros(m, dtype=bool)
    valid[inr] = (tab["flags"][nh[inr]] & cg.NEIGH_VALID).astype(bool)
    cls[~valid] = NO_NEIGH
    cls[h[:, 22] <= 1] = TTL
    if flags & cg.FWD_VERIFY_CSUM:
        cls[fold(words_be(h, 14, 10).sum(axis=1)) != 0xFFFF] = BAD_CSUM
    ihl = h[:, 14] & 15
    cls[ihl > 5] = OPTIONS
    cls[ihl < 5] = BAD_HDR
    cls[(h[:, 12] != 0x08) | (h[:, 13] != 0x00) | ((h[:, 14] >> 4) != 4)] = PASS
    cls[short] = SHORT
    return cls, nh


def rewrite_rows(h, ent):
    """Rows of frames (>= 26 bytes) rewritten with the entries ent (NEIGH_DT)."""
    h = h.copy()
    m = (h[:, 22].astype(np.int64) << 8) | h[:, 23]
    hc = (h[:, 24].astype(np.int64) << 8) | h[:, 25]
    hc2 = ~fold((~hc & 0xFFFF) + (~m & 0xFFFF) + (m - 0x0100)) & 0xFFFF
    h[:, 0:6], h[:, 6:12] = ent["dst_mac"], ent["src_mac"]
    h[:, 22] -= 1
    h[:, 24], h[:, 25] = hc2 >> 8, hc2 & 0xFF
    return h


def make_table(n_entries, seed=0):
    """Random entries; the even ones valid, every other flag bit random."""
    rng = np.random.default_rng(0xF3D0 + seed)
    t = np.zeros(n_entries, dtype=cg.NEIGH_DT)
    t.view(np.uint8)[:] = rng.integers(0, 256, t.nbytes, dtype=np.uint8)
    t["flags"] = (t["flags"] & 0xFFFE) | (np.arange(n_entries) % 2 == 0)
    return t


def set_valid_header(pk, s, ttl, corner):
    """A valid option-less IPv4 header at the frames that start at s. corner 1:
    the identification word chosen so that the checksum after the decrement is
    0x0000; corner 2: so that the checksum before it is 0x0000."""
    pk[s + 12], pk[s + 13], pk[s + 14], pk[s + 22] = 0x08, 0x00, 0x45, ttl
    rows = np.stack([pk[s + j] for j in range(34)], axis=1)
    for c in (1, 2):
        sel = corner == c
        if sel.any():
            r = rows[sel].copy()
            if c == 1:
                r[:, 22] -= 1
            w = words_be(r, 14, 10)
            w[:, 2] = w[:, 5] = 0
            ident = 0xFFFF - fold(w.sum(axis=1))
            pk[s[sel] + 18], pk[s[sel] + 19] = ident >> 8, ident & 0xFF
    rows = np.stack([pk[s + j] for j in range(34)], axis=1)
    hc = csum_full(rows)
    pk[s + 24], pk[s + 25] = hc >> 8, hc & 0xFF


class FwdCase:
    """One batch, its records, its forward lists, the check's outputs and (with_tx) its gathered bursts."""

    def __init__(self, n, layout="s64", form="dense", fwd=None, K=1, seed=0, flags=0, miss="valid", n_entries=64,
                 table=None, valid_nh=None, invalid_nh=None, exc=True, with_results=True):
        self.n, self.layout, self.form, self.K, self.flags = n, layout, form, K, flags
        self.n_lists, self.seg = (K if form == "demux" else 1), form == "seg"
        self.stride, self.data_off, self.copy_bytes, self.slot_bytes = LAYOUTS[layout]
        self.imix = self.stride == 0
        rng = np.random.default_rng(0xF0D5E + 131 * seed + n)
        m = max(n, 1)
        self.table = make_table(n_entries) if table is None else table   # the same for every case: calls share it
        self.n_entries = n_entries
        ne = n_entries
        good = np.array(valid_nh if valid_nh is not None else [x for x in range(0, min(ne, 64), 2)] +
                        [x for x in (ne - 1, ne - 2) if x >= 0 and x % 2 == 0], dtype=np.int64)
        bad = np.array(invalid_nh if invalid_nh is not None else
                       [x for x in (1, 3, ne - 1, ne - 2) if 0 <= x < ne and x % 2] +
                       [x for x in (ne, ne + 5, 0xFFFFFF) if ne <= x < (1 << 24)], dtype=np.int64)
        self.miss_nh = {"valid": int(good[-1]), "invalid": int(bad[0]) if len(bad) else cg.FWD_NO_NH,
                        "none": cg.FWD_NO_NH}[miss]
        miss_ok = miss == "valid"
        if self.imix:
            offsets = (rng.permutation(m) * 64).astype(np.uint32)
            pk = rng.integers(0, 256, m * 64 + cg.TX_MAX_FRAME + 64, dtype=np.uint8)
            starts = offsets.astype(np.int64) + self.data_off
        else:
            pk = rng.integers(0, 256, m * self.stride + (self.data_off and 64), dtype=np.uint8)
            starts = np.arange(m, dtype=np.int64) * self.stride + self.data_off
        s = starts[:n]
        i = np.arange(n)
        want = np.array(PATTERN, dtype=np.int64)[i % len(PATTERN)]
        self.prescribed = want
        # every header valid first: TTL 2, 255 and others, a quarter of each checksum corner
        ttl = np.array([2, 255, 64, 3, 128, 2, 255, 17], dtype=np.uint8)[(i // len(PATTERN) + i) % 8]
        set_valid_header(pk, s, ttl, (i // 3) % 4)
        t = want == TTL
        pk[s[t] + 22] = i[t] % 2
        x = want == BAD_HDR
        pk[s[x] + 14] = 0x40 | (i[x] % 5)
        x = want == OPTIONS
        pk[s[x] + 14] = 0x46 + (i[x] % 10)
        hdr = np.stack([pk[s + j] for j in range(34)], axis=1) if n else np.zeros((0, 34), np.uint8)
        hc = csum_full(hdr)
        fix = t | (want == BAD_HDR) | (want == OPTIONS)       # their checksums are valid too
        pk[s[fix] + 24], pk[s[fix] + 25] = hc[fix] >> 8, hc[fix] & 0xFF
        x = want == BAD_CSUM
        pk[s[x] + 24] ^= 0x01
        x = (want == PASS) & (i % 2 == 0)
        pk[s[x] + 12], pk[s[x] + 13] = 0x86, 0xDD
        x = (want == PASS) & (i % 2 == 1)
        pk[s[x] + 14] = 0x65
        lens = None
        if self.imix:
            lens = np.array(LONG_LENS, dtype=np.uint32)[np.arange(m) % len(LONG_LENS)]
            sh = np.nonzero(want == SHORT)[0]
            lens[sh] = np.array(SHORT_LENS, dtype=np.uint32)[(sh // len(PATTERN)) % len(SHORT_LENS)]
        # records: a route hit on a valid next hop, or a miss where miss_nh is valid, unless NO_NEIGH is wanted
        res = np.zeros(m, dtype=cg.RESULT_DT)
        res["verdict"], res["port"] = rng.integers(0, 5, m), rng.integers(0, 8, m)
        res["flags"] = rng.integers(0, 4, m)
        res["route_nh"] = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
        hitw = np.ones(n, dtype=bool)
        nn = want == NO_NEIGH
        if miss_ok:
            hitw = np.where(nn, True, (i // 2) % 2 == 0)
        elif len(bad) == 0:
            hitw = ~nn
        else:
            hitw = np.where(nn, (i // len(PATTERN)) % 2 == 0, True)
        if not with_results:
            assert miss_ok                                    # no records: every packet takes miss_nh
        nh = np.where(nn, bad[i % max(len(bad), 1)] if len(bad) else 0, good[i % len(good)])
        keep = want <= PASS                                   # other classes: the record is random
        setr = nn | ((want == OK) | (want == SHORT) | (want == BAD_CSUM))
        f = res["flags"][:n]
        f[setr] = (f[setr] & 0xFE) | hitw[setr]
        r = res["route_nh"][:n]
        r[setr & hitw] = (r[setr & hitw] & 0xFF000000) | nh[setr & hitw].astype(np.uint32)
        del keep
        self.starts = s
        self.inputs = {"pkts": pk, "results": res}
        if not with_results:
            del self.inputs["results"]
        if self.imix:
            self.inputs["offsets"], self.inputs["lens"] = offsets, lens
        self.with_results = with_results
        # what the builder meant, as this layout and these flags see it
        eff = want.copy()
        if not self.imix:
            eff[eff == SHORT] = OK
        if not flags & cg.FWD_VERIFY_CSUM:
            eff[eff == BAD_CSUM] = OK
        self.cls, self.nh = self.classes()
        if with_results:
            assert np.array_equal(self.cls, eff), np.nonzero(self.cls != eff)[0][:8]
        fwd = np.ones(n, dtype=bool) if fwd is None else fwd
        self.ports = (np.arange(n) // 7) % K
        idx, counts, self.true_lists = tc.lay_lists(form, n, fwd, self.ports, K)
        self.inputs["idx"], self.inputs["counts"] = idx, counts
        words = lambda k: np.full((2 * PAD) // 4 + k, GUARD * 0x01010101, dtype=np.uint32)
        o = {"out_idx": words(len(idx)), "out_count": words(len(counts)), "status": words(4 * self.n_lists)}
        if exc:
            o["exc_idx"], o["exc_count"] = words(len(idx)), words(len(counts))
        self.outs = [o]
        self.expect = [{k: v.copy() for k, v in o.items()}]
        self.tx = None

    def cfg(self) -> cg.FwdConfig:
        return cg.fwd_config(self.flags, self.miss_nh)

    def short(self, lens) -> np.ndarray:
        return np.clip(lens.astype(np.int64), 1, cg.TX_MAX_FRAME) < 34

    def classes(self):
        """(class, next hop) of every packet, from the batch as it is."""
        pk, n = self.inputs["pkts"], self.n
        s = self.inputs["offsets"][:n].astype(np.int64) + self.data_off if self.imix else \
            np.arange(n, dtype=np.int64) * self.stride + self.data_off
        h = np.stack([pk[s + j] for j in range(34)], axis=1) if n else np.zeros((0, 34), np.uint8)
        short = self.short(self.inputs["lens"][:n]) if self.imix else np.zeros(n, dtype=bool)
        res = self.inputs["results"][:n] if "results" in self.inputs else None
        return classify(h, short, res, self.table, self.n_entries, self.flags, self.miss_nh)

    def lists(self):
        """[(first word of the list in idx / out_idx, its entries as the clamps read them)]"""
        n, idx, cnt = self.n, self.inputs["idx"], self.inputs["counts"]
        if not n:
            return []
        if self.seg:
            return [(s * SEG, idx[s * SEG:s * SEG + min(int(cnt[s]), min(SEG, n - s * SEG))]) for s in range(len(cnt))]
        return [(q * n, idx[q * n:q * n + min(int(cnt[q]), n)]) for q in range(self.n_lists)]

    def expect_check(self):
        """Sets the check's part of self.expect."""
        e, o, st = self.expect[0], PAD // 4, []
        self.cls, self.nh = self.classes()
        for li, (first, ent) in enumerate(self.lists()):
            i = np.minimum(ent.astype(np.int64), self.n - 1)
            c = self.cls[i]
            keep = c <= PASS
            kept, gone = ent[keep], (i[~keep] | (c[~keep] << 28)).astype(np.uint32)
            e["out_idx"][o + first:o + first + len(kept)] = kept
            e["out_count"][o + li] = len(kept)
            if "exc_idx" in e:
                e["exc_idx"][o + first:o + first + len(gone)] = gone
                e["exc_count"][o + li] = len(gone)
            st.append((len(kept), len(gone), int((c == TTL).sum()), int((c == NO_NEIGH).sum())))
        if self.n:
            if self.seg:
                st = [tuple(np.sum(st, axis=0))]
            for q, v in enumerate(st):
                e["status"][o + 4 * q:o + 4 * q + 4] = v
        return e

    def check_status(self):
        o = PAD // 4
        return self.expect[0]["status"][o:o + 4 * self.n_lists].reshape(-1, 4)

    # ---- the rewrite: bursts as cop_tx_gather leaves them, then what the rewrite makes of them ----
    def with_tx(self, caps=None, port=True):
        pk, i = self.inputs["pkts"], self.inputs
        self.tx = tc.TxCase(pk, self.n, self.form, i["idx"], i["counts"], self.true_lists, stride=self.stride or 64,
                            data_off=self.data_off, copy_bytes=self.copy_bytes, slot_bytes=self.slot_bytes,
                            offsets=i.get("offsets"), lens=i.get("lens"), caps=caps)
        o, e = self.outs[0], self.expect[0]
        words = lambda k: np.full((2 * PAD) // 4 + k, GUARD * 0x01010101, dtype=np.uint32)
        for q, g in enumerate(self.tx.expect):
            for k, a in g.items():
                o[f"tx_{k}{q}"], e[f"tx_{k}{q}"] = a.copy(), a.copy()
            if port:
                o[f"port{q}"] = words(self.tx.caps[q][1])
                e[f"port{q}"] = o[f"port{q}"].copy()
            o[f"rw_status{q}"] = words(4)
            e[f"rw_status{q}"] = o[f"rw_status{q}"].copy()
        return self

    def expect_rewrite(self, times=1):
        """Sets the rewrite's part of self.expect (times: the call made that often)."""
        e, o = self.expect[0], PAD // 4
        res = self.inputs["results"] if "results" in self.inputs else None
        for q, L in enumerate(self.true_lists if self.n else []):
            cap_bytes, _ = self.tx.caps[q]
            fr = e[f"tx_frames{q}"]
            W = int(e[f"tx_status{q}"][o])
            Lc = np.minimum(np.asarray(L[:W], dtype=np.int64), self.n - 1)
            if self.imix:
                at = e[f"tx_off{q}"][o:o + W].astype(np.int64)
                short = e[f"tx_len{q}"][o:o + W] < 34
            else:
                at = np.arange(W, dtype=np.int64) * self.slot_bytes
                short = np.zeros(W, dtype=bool)
            short = short | (at + 48 > cap_bytes)
            for _ in range(times):
                h = np.stack([fr[PAD + at + j] for j in range(34)], axis=1) if W else np.zeros((0, 34), np.uint8)
                h[short] = 0                                  # (their bytes past the frame are never looked at)
                c, nh = classify(h, short, None if res is None else res[Lc], self.table, self.n_entries, self.flags,
                                 self.miss_nh)
                ok = c == OK
                new = rewrite_rows(h[ok], self.table[nh[ok]])
                for j in range(26):
                    fr[PAD + at[ok] + j] = new[:, j]
                if f"port{q}" in e:
                    e[f"port{q}"][o:o + W] = np.where(ok, self.table["port"][np.where(ok, nh, 0)], 0xFFFF)
                e[f"rw_status{q}"][o:o + 4] = (int(ok.sum()), int((c == PASS).sum()), int((~ok & (c != PASS)).sum()), 0)
        return e

    # ---- descriptors ----
    def descs(self, addr_in, addr_out):
        """(Batch, FwdCheckDesc, TxDesc, FwdRwDesc); addr_in(name) / addr_out(name) the base address of that array."""
        b = cg.Batch()
        if self.n:
            b.pkts, b.fwd_idx, b.fwd_count = addr_in("pkts"), addr_in("idx"), addr_in("counts")
            if self.with_results:
                b.results = addr_in("results")
        if self.imix:
            b.offsets = addr_in("offsets")
        b.n, b.stride, b.data_off = self.n, self.stride, self.data_off
        d = cg.FwdCheckDesc()
        if self.n:
            d.out_idx, d.out_count, d.status = (addr_out(k) + PAD for k in ("out_idx", "out_count", "status"))
            if "exc_idx" in self.outs[0]:
                d.exc_idx, d.exc_count = addr_out("exc_idx") + PAD, addr_out("exc_count") + PAD
            if self.imix:
                d.lens = addr_in("lens")
        t, r = cg.TxDesc(), cg.FwdRwDesc()
        if self.tx is not None:
            if self.imix and self.n:
                t.lens = addr_in("lens")
            t.copy_bytes, t.slot_bytes = self.tx.copy_bytes, self.tx.slot_bytes
            for q in range(len(self.tx.lists)):
                for k in ("frames", "off", "len", "status"):
                    setattr(t.out[q], k, addr_out(f"tx_{k}{q}") + PAD)
                t.out[q].cap_bytes, t.out[q].cap_frames = self.tx.caps[q]
                r.status[q] = addr_out(f"rw_status{q}") + PAD
                if f"port{q}" in self.outs[0]:
                    r.port[q] = addr_out(f"port{q}") + PAD
        return b, d, t, r

    def check(self, got_of):
        for k, want in self.expect[0].items():
            got = got_of(0, k)
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                raise AssertionError(f"{k} ({self.form}, n={self.n}, {self.layout}, flags={self.flags}): {len(bad)} "
                                     f"differ, first at {bad[:6]} (guard {PAD} bytes; got {got[bad[:6]]}, "
                                     f"want {want[bad[:6]]})")


def pack_descs(p: sc.Pack):
    """The four descriptor lists of a Pack of FwdCases."""
    out = [c.descs(lambda name, ci=ci: p.addr(ci, "in", 0, name), lambda k, ci=ci: p.addr(ci, "out", 0, k))
           for ci, c in enumerate(p.cases)]
    return tuple([x[j] for x in out] for j in range(4))


def host_descs(cases):
    """The four descriptor lists over the cases' own host arrays (moved to aligned memory), and a keep-alive."""
    keep, out = [], []

    def hold(a):
        keep.append(a)
        return a.ctypes.data

    for c in cases:
        c.inputs["pkts"] = sc._aligned_copy(c.inputs["pkts"])
        for k in c.outs[0]:
            c.outs[0][k] = sc._aligned_copy(c.outs[0][k])
        out.append(c.descs(lambda name, c=c: hold(c.inputs[name]), lambda k, c=c: hold(c.outs[0][k])))
    return tuple([x[j] for x in out] for j in range(4)) + (keep,)


def snapshot(cases):
    return [{**{"in:" + k: v.copy() for k, v in c.inputs.items()}, **{k: v.copy() for k, v in c.outs[0].items()}}
            for c in cases]


def unchanged(cases, snap):
    for c, s in zip(cases, snap):
        for k, v in s.items():
            now = c.inputs[k[3:]] if k.startswith("in:") else c.outs[0][k]
            assert np.array_equal(now, v), k
