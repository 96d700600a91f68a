"""Inputs and expectations the AEAD tests share (test_aead_host.py on the host,
test_gpu_aead.py on the device).

The first half restates include/cop_gpu.h "AEAD" in numpy / Python: ChaCha20
(vectorised over blocks), Poly1305 with Python integers, the frame walk and
which bytes may change. The second half builds bursts in plain numpy whose
every output extent (frames, tags, ok, status) sits between 0xAB guards;
`Burst.expect` gives what every array must hold after a seal or an open, the
guards, the gaps between frames and the skipped frames included. The same
burst runs over host memory (cop_aead_*_host) or is uploaded (Pack).
"""
import numpy as np

import copgpu as cg

GUARD = 0xAB
PAD = 64                      # guard bytes on each side of every output extent (keeps 16-byte alignment)
MAXF = cg.TX_MAX_FRAME
M64 = (1 << 64) - 1
P1305 = (1 << 130) - 5

# RFC 8439 2.8.2
RFC_KEY = bytes(range(0x80, 0xA0))
RFC_SALT = bytes.fromhex("07000000")
RFC_SEQ = 0x4746454443424140
RFC_AAD = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
RFC_TEXT = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
            b"sunscreen would be it.")
RFC_CT16 = bytes.fromhex("d31a8d34648e60db7b86afbc53ef7ec2")
RFC_TAG = bytes.fromhex("1ae10b594f09e26a7e902ecbd0600691")
RFC_EMPTY_TAG = bytes.fromhex("a0784d7a4716f3feb4f64e7f4b39bf04")

TEXT_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)
AADS = (0, 1, 12, 14, 16, 34, 64)
FRAME_COUNTS = (0, 1, 63, 64, 65, 257)


# ---- the specification, restated ------------------------------------------------------------------
def _rotl(v, n):
    return (v << np.uint32(n)) | (v >> np.uint32(32 - n))


def chacha_blocks(key: bytes, counters, nonces) -> np.ndarray:
    """ChaCha20 blocks (RFC 8439 2.3): counters (N,), nonces (N, 12) u8 -> (N, 64) u8."""
    counters = np.asarray(counters, dtype=np.uint32)
    N = len(counters)
    s = np.zeros((16, N), dtype=np.uint32)
    s[0:4] = np.array([0x61707865, 0x3320646E, 0x79622D32, 0x6B206574], dtype=np.uint32)[:, None]
    s[4:12] = np.frombuffer(key, dtype="<u4")[:, None]
    s[12] = counters
    s[13:16] = np.ascontiguousarray(np.asarray(nonces, dtype=np.uint8).reshape(N, 12)).view("<u4").T
    x = s.copy()

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    x += s
    return np.ascontiguousarray(x.T).astype("<u4").view(np.uint8).reshape(N, 64)


def nonce_of(salt: bytes, seq: int) -> bytes:
    return salt + (seq & M64).to_bytes(8, "little")


def clamp_r(otk: bytes) -> int:
    return int.from_bytes(otk[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF


def poly1305_acc(otk: bytes, msg: bytes) -> int:
    """The accumulator after the last block, reduced mod 2^130 - 5 (what the final addition of s sees)."""
    r, h = clamp_r(otk), 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        h = (h + int.from_bytes(blk + b"\x01", "little")) * r % P1305
    return h


def poly1305(otk: bytes, msg: bytes) -> bytes:
    """RFC 8439 2.5 with Python integers."""
    s = int.from_bytes(otk[16:], "little")
    return ((poly1305_acc(otk, msg) + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


def aead_tag(otk: bytes, ad: bytes, ct: bytes) -> bytes:
    return poly1305(otk, pad16(ad) + pad16(ct) + len(ad).to_bytes(8, "little") + len(ct).to_bytes(8, "little"))


def seal_frame(key: bytes, salt: bytes, seq: int, frame: bytes, aad_bytes: int):
    """(frame after seal, tag) of one frame under sequence number seq."""
    l = len(frame)
    a = min(aad_bytes, l)
    nb = 1 + (l - a + 63) // 64
    assert nb <= 33                                   # counter 0 .. 32: no counter wrap exists
    blocks = chacha_blocks(key, np.arange(nb), np.tile(np.frombuffer(nonce_of(salt, seq), np.uint8), (nb, 1)))
    ks = blocks[1:].reshape(-1)[:l - a]
    ct = (np.frombuffer(frame[a:], np.uint8) ^ ks).tobytes()
    return frame[:a] + ct, aead_tag(blocks[0, :32].tobytes(), frame[:a], ct)


def open_frame(key: bytes, salt: bytes, seq: int, frame: bytes, aad_bytes: int, tag: bytes):
    """(frame after open, ok)."""
    l = len(frame)
    a = min(aad_bytes, l)
    nb = 1 + (l - a + 63) // 64
    blocks = chacha_blocks(key, np.arange(nb), np.tile(np.frombuffer(nonce_of(salt, seq), np.uint8), (nb, 1)))
    if aead_tag(blocks[0, :32].tobytes(), frame[:a], frame[a:]) != tag:
        return frame, 0
    ks = blocks[1:].reshape(-1)[:l - a]
    return frame[:a] + (np.frombuffer(frame[a:], np.uint8) ^ ks).tobytes(), 1


# ---- bursts ---------------------------------------------------------------------------------------
def words(m: int) -> np.ndarray:
    return np.full((PAD + 4 * m + PAD) // 4, GUARD * 0x01010101, dtype=np.uint32)


class Burst:
    """One cop_aead_burst in numpy. lens given: the off / len form (frames laid
    end to end at their ext, `gap` spare bytes between them); else the slot
    form. count: the value of *count, or None for a NULL count. bad: {k:
    "misaligned" | "past"} moves off[k] so that frame k is skipped (off / len
    form). cap_cut: bytes taken off cap_bytes (slot form: the last frames no
    longer fit)."""

    def __init__(self, n, aad, lens=None, frame_bytes=0, slot_bytes=0, seq_base=0, count=None, bad=None, gap=0,
                 cap_cut=0, seed=1, key=None, salt=b"\0\0\0\0"):
        rng = np.random.default_rng(0xAEAD00 + seed)
        self.n, self.aad, self.seq_base, self.count = n, aad, seq_base, count
        self.key = bytes(rng.integers(0, 256, 32, dtype=np.uint8)) if key is None else key
        self.salt = salt
        self.form = "slot" if lens is None else "offlen"
        self.frame_bytes, self.slot_bytes = frame_bytes, (slot_bytes or ((frame_bytes + 15) & ~15))
        self.arr = {}
        if lens is None:
            self.frame_bytes, self.slot_bytes = frame_bytes, self.slot_bytes
            cap = n * self.slot_bytes
        else:
            lens = np.asarray(lens, dtype=np.uint32)
            assert len(lens) == n
            ext = (np.minimum(lens, MAXF).astype(np.int64) + 15) & ~15
            off = np.cumsum(ext + gap) - (ext + gap)
            cap = int(off[-1] + ext[-1]) if n else 0
            off = off.astype(np.uint32)
            for k, how in (bad or {}).items():
                off[k] = off[k] + 8 if how == "misaligned" else cap - int(ext[k]) + 16
            self.frame_bytes = self.slot_bytes = 0
            self.arr["off"], self.arr["len"] = (np.concatenate([off, [0]]).astype(np.uint32)[:max(n, 1)],
                                                np.concatenate([lens, [0]]).astype(np.uint32)[:max(n, 1)])
        self.cap = max(cap - cap_cut, 0)
        fr = np.full(PAD + max(self.cap, 16) + PAD, GUARD, dtype=np.uint8)
        fr[PAD:PAD + self.cap] = rng.integers(0, 256, self.cap, dtype=np.uint8)
        self.arr["frames"] = fr
        if count is not None:
            self.arr["count"] = np.array([count], dtype=np.uint32)
        self.arr["tags"] = np.full(PAD + 16 * max(n, 1) + PAD, GUARD, dtype=np.uint8)
        self.arr["ok"] = words(max(n, 1))
        self.arr["status"] = words(4)

    # the walk of include/cop_gpu.h
    def present(self) -> int:
        return self.n if self.count is None else min(self.count, self.n)

    def walk(self):
        """[(k, o, l) or (k, None, None) if skipped] for k < frames present."""
        out = []
        for k in range(self.present()):
            if self.form == "slot":
                o, l = k * self.slot_bytes, self.frame_bytes
            else:
                o, l = int(self.arr["off"][k]), min(int(self.arr["len"][k]), MAXF)
            ext = (l + 15) & ~15
            out.append((k, None, None) if (o % 16 or o + ext > self.cap) else (k, o, l))
        return out

    def frame(self, k, arr=None):
        """Frame k's bytes [0, l) (None if skipped)."""
        fr = self.arr["frames"] if arr is None else arr
        for kk, o, l in self.walk():
            if kk == k:
                return None if o is None else fr[PAD + o:PAD + o + l].tobytes()
        return None

    def expect(self, mode: str) -> dict:
        """The arrays after cop_aead_seal ("seal") or cop_aead_open ("open") of the arrays as they are."""
        e = {k: v.copy() for k, v in self.arr.items()}
        if not self.n:
            return e                                          # skipped whole
        done = bad = skipped = 0
        for k, o, l in self.walk():
            if o is None:
                skipped += 1
                continue
            done += 1
            f = self.arr["frames"][PAD + o:PAD + o + l].tobytes()
            seq = self.seq_base + k
            if mode == "seal":
                g, tag = seal_frame(self.key, self.salt, seq, f, self.aad)
                e["tags"][PAD + 16 * k:PAD + 16 * k + 16] = np.frombuffer(tag, np.uint8)
            else:
                g, ok = open_frame(self.key, self.salt, seq, f, self.aad,
                                   self.arr["tags"][PAD + 16 * k:PAD + 16 * k + 16].tobytes())
                e["ok"][PAD // 4 + k] = ok
                bad += 1 - ok
            assert g[:min(self.aad, l)] == f[:min(self.aad, l)]
            e["frames"][PAD + o:PAD + o + l] = np.frombuffer(g, np.uint8)
        e["status"][PAD // 4:PAD // 4 + 4] = (done, bad, skipped, 0)
        return e

    def expect_poly(self, otk: np.ndarray) -> dict:
        """After cop_poly1305_bulk with otk (n, 32) u8."""
        e = {k: v.copy() for k, v in self.arr.items()}
        done = skipped = 0
        for k, o, l in self.walk():
            if o is None:
                skipped += 1
                continue
            done += 1
            tag = poly1305(otk[k].tobytes(), self.arr["frames"][PAD + o:PAD + o + l].tobytes())
            e["tags"][PAD + 16 * k:PAD + 16 * k + 16] = np.frombuffer(tag, np.uint8)
        e["status"][PAD // 4:PAD // 4 + 4] = (done, 0, skipped, 0)
        return e

    def desc(self, addr_of, mode: str) -> "cg.AeadBurst":
        """The cop_aead_burst, addr_of(name) the base address of that array (outputs: of its guard)."""
        g = lambda name: addr_of(name) + PAD
        return cg.make_aead_burst(g("frames"), g("tags"), g("status"), self.n, self.cap,
                                  off=addr_of("off") if "off" in self.arr else None,
                                  len=addr_of("len") if "len" in self.arr else None,
                                  count=addr_of("count") if "count" in self.arr else None,
                                  ok=g("ok") if mode == "open" else None, seq_base=self.seq_base,
                                  slot_bytes=self.slot_bytes, frame_bytes=self.frame_bytes, aad_bytes=self.aad)

    def cg_key(self):
        return cg.aead_key(self.key, self.salt)

    def compare(self, want: dict, got_of=None):
        for name, w in want.items():
            got = self.arr[name] if got_of is None else got_of(name)
            if not np.array_equal(got, w):
                bad = np.nonzero(got != w)[0]
                st = (self.arr["status"] if got_of is None else got_of("status"))[PAD // 4:PAD // 4 + 4]
                raise AssertionError(f"{name}: {len(bad)} differ, first at {bad[:6]} (guard {PAD} bytes; got "
                                     f"{got[bad[:6]]}, want {w[bad[:6]]}); status got {st} want "
                                     f"{want['status'][PAD // 4:PAD // 4 + 4]}; n={self.n} aad={self.aad} {self.form}")


def aligned(b: Burst) -> Burst:
    """Move the burst's arrays into 64-byte aligned host memory."""
    for name, a in list(b.arr.items()):
        raw = np.zeros(a.nbytes + 64, dtype=np.uint8)
        o = (-raw.ctypes.data) % 64
        v = raw[o:o + a.nbytes]
        v[:] = a.view(np.uint8)
        b.arr[name] = v.view(a.dtype)
    return b


def run_host(bursts, mode: str, key=None) -> int:
    """cop_aead_seal_host / _open_host over the bursts' own arrays (one call, one key). The C code."""
    ds = [b.desc(lambda name, b=b: b.arr[name].ctypes.data, mode) for b in bursts]
    key = key or (bursts[0].cg_key() if bursts else cg.aead_key(bytes(32)))
    return (cg.aead_seal_host if mode == "seal" else cg.aead_open_host)(key, ds)


def imix_lens(n: int, seed: int = 3) -> np.ndarray:
    """Lengths of every kind in a shuffled order: the short ones, each 16-byte phase, 7:4:1 IMIX, the clamp."""
    kinds = np.array([1, 15, 16, 17, 60, 64, 65, 127, 128, 129, 594, 1518, 2047, 2048, 5000, 64, 64, 594], dtype=np.uint32)
    return kinds[np.random.default_rng(seed).integers(0, len(kinds), n)]


def matrix():
    """(name, Burst) of the case matrix both suites run: every text length at every aad, frame counts,
    both forms, counts, skipped frames, sequence carries."""
    out = []
    for i, aad in enumerate(AADS + (4000,)):                     # 4000 is refused: replaced below by aad >= l
        a = 300 if aad == 4000 else aad
        lens = [min(a, 300) + t for t in TEXT_LENS] + [MAXF] + ([5000] if i % 2 else [])
        if aad == 4000:
            lens = [1, 16, 17, 300, 299]                          # aad >= l: authenticated only
        out.append((f"lens@aad={a}", Burst(len(lens), a, lens=lens, seq_base=7 + i, seed=i, gap=16 * (i % 2))))
    for t in (0, 1, 17, 64, 129, MAXF - 34):
        out.append((f"slot:text={t}", Burst(5, 34, frame_bytes=34 + t, slot_bytes=((34 + t + 15) & ~15) + 32 * (t % 2),
                                            seq_base=1 << 40, seed=40 + t)))
    for n in FRAME_COUNTS:
        out.append((f"slot:n={n}", Burst(n, 34, frame_bytes=64, slot_bytes=64, seed=100 + n, salt=b"\1\2\3\4")))
        out.append((f"offlen:n={n}", Burst(n, 14, lens=imix_lens(n, n), seed=200 + n)))
    for name, cnt in (("below", 40), ("equal", 65), ("above", 1000), ("zero", 0)):
        out.append((f"count:{name}", Burst(65, 12, lens=imix_lens(65, 9), count=cnt, seed=300 + cnt % 7)))
        out.append((f"count:{name}:slot", Burst(65, 16, frame_bytes=80, slot_bytes=96, count=cnt, seed=310 + cnt % 7)))
    out.append(("skipped", Burst(70, 34, lens=imix_lens(70, 4), bad={0: "misaligned", 33: "past", 34: "misaligned",
                                                                      69: "past"}, seed=400)))
    out.append(("slot:cap_cut", Burst(9, 34, frame_bytes=100, slot_bytes=128, cap_cut=128 + 20, seed=401)))
    for sb in ((1 << 32) - 2, (1 << 64) - 2):                     # carry into the high nonce word; the wrap
        out.append((f"seq_base={sb:#x}", Burst(5, 34, frame_bytes=64, slot_bytes=64, seq_base=sb, seed=500)))
    return out


# ---- Poly1305 edge keys and messages -----------------------------------------------------------------
def poly_edges():
    """(name, otk, msg): the carry cases no key derived from ChaCha reaches."""
    rng = np.random.default_rng(0x1305)
    rnd = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))
    ff = b"\xff" * 16
    out = []
    for rname, r in (("r=ff", ff), ("r=0", bytes(16)), ("r=rnd", rnd(16))):
        for sname, s in (("s=ff", ff), ("s=rnd", rnd(16))):
            for nblk in range(1, 9):
                out.append((f"{rname},{sname},ff*{nblk}", r + s, ff * nblk))
            for nbytes in (15, 17):
                out.append((f"{rname},{sname},ff[{nbytes}]", r + s, b"\xff" * nbytes))
            out.append((f"{rname},{sname},empty", r + s, b""))
    # messages that leave the accumulator in [2^130 - 5, 2^130) before the final reduction
    r1 = (1).to_bytes(16, "little")
    for d in range(5):
        out.append((f"acc=p+{d}", r1 + rnd(16), top_band_message(d)))
    return out


def top_band_message(d: int) -> bytes:
    """With r = 1 (its clamped value too) the accumulator is the plain sum of the blocks, each with
    its 2^128 bit, and no step reduces it while it stays below 2^130. Two blocks 2^128 + m_i with
    m_1 + m_2 = 2^129 - 5 + d sum to 2^130 - 5 + d for d < 4; three blocks reach 2^130 - 1 (d = 4)."""
    top = (1 << 128) - 1
    ms = [top, top - 3 + d] if d < 4 else [top, 0, 0]
    msg = b"".join(m.to_bytes(16, "little") for m in ms)
    acc = sum(int.from_bytes(msg[i:i + 16] + b"\x01", "little") for i in range(0, len(msg), 16))
    assert P1305 <= acc < (1 << 130) and acc - P1305 == d == poly1305_acc(r1_otk(), msg)
    return msg


def r1_otk() -> bytes:
    return (1).to_bytes(16, "little") + bytes(16)


# ---- OpenSSL's libcrypto, the independent implementation (host tests, the golden generator) -----------
class OpenSSL:
    """EVP_chacha20_poly1305 and the POLY1305 EVP_MAC through ctypes; OpenSSL.load() is None where
    libcrypto (3.x) is absent."""
    _inst = False

    @classmethod
    def load(cls):
        if cls._inst is False:
            try:
                cls._inst = cls()
            except (OSError, AttributeError, TypeError):
                cls._inst = None
        return cls._inst

    def __init__(self):
        import ctypes
        import ctypes.util
        C = self.C = ctypes
        L = self.L = C.CDLL(ctypes.util.find_library("crypto"))
        vp, ci, cp = C.c_void_p, C.c_int, C.c_char_p
        for name, res, args in (("EVP_CIPHER_CTX_new", vp, []), ("EVP_CIPHER_CTX_free", None, [vp]),
                                ("EVP_chacha20_poly1305", vp, []),
                                ("EVP_EncryptInit_ex", ci, [vp, vp, vp, cp, cp]),
                                ("EVP_EncryptUpdate", ci, [vp, cp, C.POINTER(ci), cp, ci]),
                                ("EVP_EncryptFinal_ex", ci, [vp, cp, C.POINTER(ci)]),
                                ("EVP_CIPHER_CTX_ctrl", ci, [vp, ci, ci, vp]),
                                ("EVP_MAC_fetch", vp, [vp, cp, cp]), ("EVP_MAC_free", None, [vp]),
                                ("EVP_MAC_CTX_new", vp, [vp]), ("EVP_MAC_CTX_free", None, [vp]),
                                ("EVP_MAC_init", ci, [vp, cp, C.c_size_t, vp]),
                                ("EVP_MAC_update", ci, [vp, cp, C.c_size_t]),
                                ("EVP_MAC_final", ci, [vp, cp, C.POINTER(C.c_size_t), C.c_size_t])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        self.mac = L.EVP_MAC_fetch(None, b"POLY1305", None)
        if not self.mac:
            raise OSError("no POLY1305 EVP_MAC")
        assert self.poly1305(bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b"),
                             b"Cryptographic Forum Research Group").hex() == "a8061dc1305136c6c22b8baf0c0127a9"

    def seal(self, key: bytes, nonce: bytes, aad: bytes, text: bytes):
        """(ciphertext, tag)."""
        C, L = self.C, self.L
        ctx = L.EVP_CIPHER_CTX_new()
        try:
            n = C.c_int(0)
            out = C.create_string_buffer(len(text) + 16)
            tag = C.create_string_buffer(16)
            ok = L.EVP_EncryptInit_ex(ctx, L.EVP_chacha20_poly1305(), None, None, None)
            ok &= L.EVP_CIPHER_CTX_ctrl(ctx, 0x9, 12, None)                   # EVP_CTRL_AEAD_SET_IVLEN
            ok &= L.EVP_EncryptInit_ex(ctx, None, None, key, nonce)
            if aad:
                ok &= L.EVP_EncryptUpdate(ctx, None, C.byref(n), aad, len(aad))
            total = 0
            if text:
                ok &= L.EVP_EncryptUpdate(ctx, out, C.byref(n), text, len(text))
                total = n.value
            ok &= L.EVP_EncryptFinal_ex(ctx, C.cast(C.addressof(out) + total, C.c_char_p), C.byref(n))
            ok &= L.EVP_CIPHER_CTX_ctrl(ctx, 0x10, 16, C.cast(tag, C.c_void_p))   # EVP_CTRL_AEAD_GET_TAG
            assert ok == 1 and total + n.value == len(text)
            return out.raw[:len(text)], tag.raw
        finally:
            L.EVP_CIPHER_CTX_free(ctx)

    def poly1305(self, otk: bytes, msg: bytes) -> bytes:
        C, L = self.C, self.L
        ctx = L.EVP_MAC_CTX_new(self.mac)
        try:
            out, n = C.create_string_buffer(16), C.c_size_t(0)
            ok = L.EVP_MAC_init(ctx, otk, 32, None)
            if msg:
                ok &= L.EVP_MAC_update(ctx, msg, len(msg))
            ok &= L.EVP_MAC_final(ctx, out, C.byref(n), 16)
            assert ok == 1 and n.value == 16
            return out.raw
        finally:
            L.EVP_MAC_CTX_free(ctx)
