"""cop_aead_*_host, cop_poly1305_host and cop_chacha20_block_host (csrc/aead.c)
against the numpy / Python restatement in aead_cases.py, and both against
OpenSSL's libcrypto (EVP_chacha20_poly1305, the POLY1305 EVP_MAC) through
ctypes: no code of this project agrees with itself alone. The OpenSSL checks,
and only they, skip where libcrypto is absent; tests/golden/aead/aead_vectors.npz
holds its recorded outputs for the machines without it.

Every output extent sits between 0xAB guards and whole arrays are compared, so
a byte written outside a processed frame's text, a tag or ok word at or past the
frame count, or anything of a skipped frame shows.

The ChaCha block counter of a frame is 0 for the one-time key and 1 .. 32 for
at most COP_TX_MAX_FRAME = 2048 bytes of text: it stays below 33, so no counter
wrap exists (aead_cases.seal_frame asserts it).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aead_cases as ac
import copgpu as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
PAD = ac.PAD
ssl = ac.OpenSSL.load()
needs_openssl = pytest.mark.skipif(ssl is None, reason="no libcrypto with EVP_chacha20_poly1305 and POLY1305")

MATRIX = ac.matrix()


def sealed(b: ac.Burst) -> ac.Burst:
    assert ac.run_host([ac.aligned(b)], "seal") == 0
    return b


# ---- the building blocks -------------------------------------------------------------------------------
def test_chacha20_block_against_the_rfc_and_the_restatement():
    key, nonce = bytes(range(32)), bytes.fromhex("000000090000004a00000000")
    want = ("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
            "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    assert cg.chacha20_block_host(key, 1, nonce).hex() == want
    rng = np.random.default_rng(20)
    for ctr in (0, 1, 32, 0xFFFFFFFF):
        k, n = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 12, dtype=np.uint8))
        assert cg.chacha20_block_host(k, ctr, n) == ac.chacha_blocks(k, [ctr], np.frombuffer(n, np.uint8)[None])[0].tobytes()


def test_poly1305_edges_against_the_restatement():
    for name, otk, msg in ac.poly_edges():
        assert cg.poly1305_host(otk, msg) == ac.poly1305(otk, msg), name
    for d in range(5):      # the accumulator lands d above 2^130 - 5: the tag is d + s
        otk = ac.r1_otk()[:16] + bytes([0xF0] * 16)
        want = ((d + int.from_bytes(otk[16:], "little")) & ((1 << 128) - 1)).to_bytes(16, "little")
        assert cg.poly1305_host(otk, ac.top_band_message(d)) == want


@needs_openssl
def test_poly1305_edges_against_openssl():
    for name, otk, msg in ac.poly_edges():
        assert cg.poly1305_host(otk, msg) == ssl.poly1305(otk, msg), name
    rng = np.random.default_rng(21)
    for n in (1, 16, 31, 32, 33, 257, 2048):
        otk, msg = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, n, dtype=np.uint8))
        assert cg.poly1305_host(otk, msg) == ssl.poly1305(otk, msg) == ac.poly1305(otk, msg), n


# ---- RFC 8439 2.8.2 through the API -----------------------------------------------------------------------
def rfc_burst(frame: bytes, aad: int) -> ac.Burst:
    b = ac.Burst(1, aad, lens=[len(frame)], seq_base=ac.RFC_SEQ, key=ac.RFC_KEY, salt=ac.RFC_SALT)
    b.arr["frames"][PAD:PAD + len(frame)] = np.frombuffer(frame, np.uint8)
    return b


def test_rfc_vector():
    b = sealed(rfc_burst(ac.RFC_AAD + ac.RFC_TEXT, 12))
    f = b.arr["frames"][PAD:PAD + 126].tobytes()
    assert f[:12] == ac.RFC_AAD and f[12:28] == ac.RFC_CT16
    assert b.arr["tags"][PAD:PAD + 16].tobytes() == ac.RFC_TAG
    assert list(b.arr["status"][PAD // 4:PAD // 4 + 4]) == [1, 0, 0, 0]
    assert ac.run_host([b], "open") == 0
    assert b.arr["frames"][PAD:PAD + 126].tobytes() == ac.RFC_AAD + ac.RFC_TEXT and b.arr["ok"][PAD // 4] == 1
    e = sealed(rfc_burst(b"", 0))                      # empty AAD, empty text
    assert e.arr["tags"][PAD:PAD + 16].tobytes() == ac.RFC_EMPTY_TAG


# ---- the case matrix -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in MATRIX])
def test_mirror_against_the_restatement(name):
    b = ac.aligned(dict(ac.matrix())[name])
    plain = {k: v.copy() for k, v in b.arr.items()}
    want = b.expect("seal")
    assert ac.run_host([b], "seal") == 0
    b.compare(want)
    want = b.expect("open")
    assert ac.run_host([b], "open") == 0
    b.compare(want)
    assert np.array_equal(b.arr["frames"], plain["frames"])          # seal then open restores every byte
    st = b.arr["status"][PAD // 4:PAD // 4 + 4]
    if b.n:
        assert st[0] + st[2] == b.present() and st[1] == 0


@needs_openssl
def test_restatement_and_mirror_against_openssl():
    """Every frame of the length x aad bursts, of the IMIX burst and of the sequence-number bursts."""
    seen = 0
    for name, b in MATRIX:
        if not name.startswith(("lens@", "offlen:n=65", "seq_base", "slot:text")):
            continue
        plain = b.arr["frames"].copy()
        sealed(b)
        for k, o, l in b.walk():
            f = plain[PAD + o:PAD + o + l].tobytes()
            a = min(b.aad, l)
            ct, tag = ssl.seal(b.key, ac.nonce_of(b.salt, b.seq_base + k), f[:a], f[a:])
            assert b.arr["frames"][PAD + o:PAD + o + l].tobytes() == f[:a] + ct, (name, k)
            assert b.arr["tags"][PAD + 16 * k:PAD + 16 * k + 16].tobytes() == tag, (name, k)
            assert ac.seal_frame(b.key, b.salt, b.seq_base + k, f, b.aad) == (f[:a] + ct, tag), (name, k)
            seen += 1
    assert seen > 200


def test_several_bursts_in_one_call():
    key = bytes(range(32))
    bs = [ac.aligned(ac.Burst(65, 34, frame_bytes=64, slot_bytes=64, seed=1, key=key, seq_base=0)),
          ac.aligned(ac.Burst(0, 34, frame_bytes=64, slot_bytes=64, seed=2, key=key)),
          ac.aligned(ac.Burst(40, 14, lens=ac.imix_lens(40), seed=3, key=key, seq_base=65, count=33)),
          ac.aligned(ac.Burst(7, 0, frame_bytes=1518, slot_bytes=1520, seed=4, key=key, seq_base=1 << 33))]
    for mode in ("seal", "open"):
        want = [b.expect(mode) for b in bs]
        assert ac.run_host(bs, mode) == 0
        for b, w in zip(bs, want):
            b.compare(w)


# ---- open: forged frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["text", "aad", "tag", "seq_base", "key", "salt"])
def test_one_flipped_bit_fails_the_frame_and_leaves_it(what):
    b = sealed(ac.Burst(9, 34, lens=[64, 98, 594, 34, 35, 1518, 60, 2048, 64], seed=77, seq_base=1000))
    hit = {"text": [1, 5], "aad": [2, 3], "tag": [0, 8]}.get(what, list(range(9)))
    walk = {k: (o, l) for k, o, l in b.walk()}
    if what == "text":
        for k in hit:
            b.arr["frames"][PAD + walk[k][0] + walk[k][1] - 1] ^= 0x01
    elif what == "aad":
        for k in hit:
            b.arr["frames"][PAD + walk[k][0] + 33] ^= 0x80
    elif what == "tag":
        for k in hit:
            b.arr["tags"][PAD + 16 * k + (15 if k else 0)] ^= 0x04
    elif what == "seq_base":
        b.seq_base ^= 1
    elif what == "key":
        b.key = bytes([b.key[0] ^ 1]) + b.key[1:]
    else:
        b.salt = b"\0\0\0\x80"
    before = b.arr["frames"].copy()
    want = b.expect("open")
    assert ac.run_host([b], "open") == 0
    b.compare(want)
    ok = b.arr["ok"][PAD // 4:PAD // 4 + 9]
    assert [k for k in range(9) if not ok[k]] == hit
    assert list(b.arr["status"][PAD // 4:PAD // 4 + 4]) == [9, len(hit), 0, 0]
    for k in hit:                                           # byte-identical to its input
        o, l = walk[k]
        assert np.array_equal(b.arr["frames"][PAD + o:PAD + o + l], before[PAD + o:PAD + o + l])


# ---- the golden file ---------------------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "aead", "aead_vectors.npz"))


def test_golden_vectors_against_the_mirror():
    g = golden()
    assert 20 <= len(g["len"]) <= 40 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "aead", "aead_vectors.npz")) < 65536
    for i in range(len(g["len"])):
        l, s = int(g["len"][i]), int(g["start"][i])
        b = ac.Burst(1, int(g["aad"][i]), lens=[l], seq_base=int(g["seq"][i]), key=g["key"][i].tobytes(),
                     salt=g["salt"][i].tobytes())
        b.arr["frames"][PAD:PAD + l] = g["plain"][s:s + l]
        sealed(b)
        assert np.array_equal(b.arr["frames"][PAD:PAD + l], g["sealed"][s:s + l]), i
        assert np.array_equal(b.arr["tags"][PAD:PAD + 16], g["tag"][i]), i
    for i in range(len(g["mlen"])):
        m = g["msg"][int(g["mstart"][i]):int(g["mstart"][i]) + int(g["mlen"][i])].tobytes()
        assert cg.poly1305_host(g["otk"][i].tobytes(), m) == g["ptag"][i].tobytes(), i


@needs_openssl
def test_golden_vectors_are_what_openssl_gives():
    g = golden()
    for i in range(len(g["len"])):
        l, s, a = int(g["len"][i]), int(g["start"][i]), min(int(g["aad"][i]), int(g["len"][i]))
        f = g["plain"][s:s + l].tobytes()
        ct, tag = ssl.seal(g["key"][i].tobytes(), ac.nonce_of(g["salt"][i].tobytes(), int(g["seq"][i])), f[:a], f[a:])
        assert f[:a] + ct == g["sealed"][s:s + l].tobytes() and tag == g["tag"][i].tobytes(), i
    for i in range(len(g["mlen"])):
        m = g["msg"][int(g["mstart"][i]):int(g["mstart"][i]) + int(g["mlen"][i])].tobytes()
        assert ssl.poly1305(g["otk"][i].tobytes(), m) == g["ptag"][i].tobytes(), i


# ---- errors --------------------------------------------------------------------------------------------------
def error_mutations():
    """(name, mode, mutate(desc, burst)) of every -EINVAL a single burst can give."""
    def setf(field, value):
        def mut(d, b):
            setattr(d, field, value(getattr(d, field), d) if callable(value) else value)
        return mut
    slot = [("frames NULL", "seal", setf("frames", None)), ("tags NULL", "seal", setf("tags", None)),
            ("status NULL", "seal", setf("status", None)), ("ok NULL in open", "open", setf("ok", None)),
            ("ok in seal", "seal", setf("ok", lambda v, d: d.status + 256)),
            ("frame_bytes 0", "seal", setf("frame_bytes", 0)), ("frame_bytes 2049", "seal", setf("frame_bytes", 2049)),
            ("slot_bytes 72", "seal", setf("slot_bytes", 72)), ("slot_bytes < frame_bytes", "seal", setf("slot_bytes", 48)),
            ("aad_bytes 2049", "seal", setf("aad_bytes", 2049)), ("frames + 8", "seal", setf("frames", lambda v, d: v + 8)),
            ("tags + 4", "seal", setf("tags", lambda v, d: v + 4)), ("status + 8", "open", setf("status", lambda v, d: v + 8)),
            ("cap_bytes 2^32", "seal", setf("cap_bytes", 1 << 32)),
            ("tags in frames", "seal", setf("tags", lambda v, d: d.frames + 64)),
            ("status in frames", "seal", setf("status", lambda v, d: d.frames + d.cap_bytes - 16)),
            ("ok in frames", "open", setf("ok", lambda v, d: d.frames)),
            ("status in tags", "seal", setf("status", lambda v, d: d.tags + 16)),
            ("ok over status", "open", setf("ok", lambda v, d: d.status - 8)),
            ("count in tags", "seal", setf("count", lambda v, d: d.tags + 32))]
    offlen = [("len without off", "seal", setf("off", None)), ("off without len", "open", setf("len", None)),
              ("tags over off", "seal", setf("tags", lambda v, d: d.off & ~15)),
              ("status over len", "seal", setf("status", lambda v, d: d.len & ~15)),
              ("status over count", "open", setf("status", lambda v, d: d.count & ~15)),
              ("off misaligned", "seal", setf("off", lambda v, d: v + 2))]
    return slot, offlen


def test_einval_leaves_every_array_alone():
    slot, offlen = error_mutations()
    for muts, make in ((slot, lambda: ac.Burst(5, 34, frame_bytes=64, slot_bytes=64, seed=9)),
                       (offlen, lambda: ac.Burst(5, 34, lens=[64, 65, 1, 2048, 16], count=5, seed=9))):
        for name, mode, mut in muts:
            b = ac.aligned(make())
            # off, len and count in one aligned block, so that an extent put over them is aligned
            before = {k: v.copy() for k, v in b.arr.items()}
            d = b.desc(lambda nm: b.arr[nm].ctypes.data, mode)
            mut(d, b)
            f = cg.aead_seal_host if mode == "seal" else cg.aead_open_host
            assert f(b.cg_key(), [d]) == EINVAL, name
            for k, v in before.items():
                assert np.array_equal(b.arr[k], v), (name, k)
    # another burst's extents
    a, c = ac.aligned(ac.Burst(5, 34, frame_bytes=64, slot_bytes=64, seed=1)), ac.aligned(ac.Burst(5, 34, frame_bytes=64, slot_bytes=64, seed=2))
    da, dc = (x.desc(lambda nm, x=x: x.arr[nm].ctypes.data, "seal") for x in (a, c))
    for field, value in (("tags", da.tags), ("status", da.status), ("frames", da.frames + 64), ("status", da.frames + 16)):
        d2 = c.desc(lambda nm: c.arr[nm].ctypes.data, "seal")
        setattr(d2, field, value)
        before = [x.arr["frames"].copy() for x in (a, c)]
        assert cg.aead_seal_host(a.cg_key(), [da, d2]) == EINVAL, field
        assert all(np.array_equal(x.arr["frames"], w) for x, w in zip((a, c), before))
    assert dc.n_frames == 5
    # nothing to do: 0, nothing needed
    assert cg.aead_seal_host(a.cg_key(), []) == 0
    empty = cg.make_aead_burst(None, None, None, 0, 0)
    assert cg.aead_seal_host(a.cg_key(), [empty]) == 0 and cg.aead_open_host(a.cg_key(), [empty]) == 0


# ---- layouts, sanitizers ----------------------------------------------------------------------------------------
def test_struct_layouts_match_c(tmp_path):
    """AeadKey / AeadBurst have the C compiler's size and field offsets."""
    mirrors = {"cop_aead_key": cg.AeadKey, "cop_aead_burst": cg.AeadBurst}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cop_gpu.h"', "int main(void){"]
    for cname, py in mirrors.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("consts %u\\n", COP_AEAD_TAG_BYTES * 10000 + COP_TX_MAX_FRAME);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(l.split()[:-1]): int(l.split()[-1]) for l in out if l.strip()}
    for cname, py in mirrors.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert got[("consts",)] == cg.AEAD_TAG_BYTES * 10000 + cg.TX_MAX_FRAME


def test_aead_under_sanitizers(tmp_path):
    """tests/c/aead_check.c, a stand-alone program: aead.c built with
    -fsanitize=address,undefined over exactly sized heap blocks, so a byte read
    or written outside an extent stops it."""
    exe = tmp_path / "aead_check"
    csrc = os.path.join(ROOT, "ghost-dataplane_amd", "csrc")
    cc = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", csrc,
                         os.path.join(ROOT, "tests", "c", "aead_check.c"), os.path.join(csrc, "aead.c"), os.path.join(csrc, "extents.c"),
                         "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "aead_check ok" in run.stdout
