"""Writes tests/golden/aead/aead_vectors.npz: what OpenSSL's libcrypto gives for two
dozen of the AEAD cases (EVP_chacha20_poly1305) and for the Poly1305 edge keys
(the POLY1305 EVP_MAC), so that the GPU tests have an independent expectation
on a machine with neither OpenSSL nor anything else to compare with. The file
has a folder of its own because the pipeline's golden tests take every *.npz
directly under tests/golden/ for a pipeline fixture.

    python tests/golden/make_aead_golden.py

Frames: key (N, 32), salt (N, 4), seq (N,) u64, aad (N,) = aad_bytes, len (N,),
start (N,) = the frame's first byte in `plain` / `sealed` (the frames end to
end, each padded to 16 bytes), tag (N, 16). Poly1305: otk (M, 32), mlen (M,),
mstart (M,), msg (the messages padded likewise), ptag (M, 16).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "ghost-dataplane_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import aead_cases as ac  # noqa: E402


def main():
    ssl = ac.OpenSSL.load()
    if ssl is None:
        raise SystemExit("libcrypto with EVP_chacha20_poly1305 and the POLY1305 EVP_MAC is needed")
    rng = np.random.default_rng(0x601DE4)
    frames = [(ac.RFC_KEY, ac.RFC_SALT, ac.RFC_SEQ, 12, ac.RFC_AAD + ac.RFC_TEXT),
              (ac.RFC_KEY, ac.RFC_SALT, ac.RFC_SEQ, 0, b"")]
    shapes = [(0, 1), (0, 64), (1, 17), (12, 12), (12, 13), (14, 64), (14, 78), (16, 16), (16, 80), (34, 64), (34, 60),
              (34, 98), (34, 99), (34, 594), (34, 1518), (64, 64), (64, 191), (64, 193), (34, 2048), (0, 2048),
              (300, 299), (14, 271)]
    for i, (aad, l) in enumerate(shapes):
        key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        salt = bytes(rng.integers(0, 256, 4, dtype=np.uint8)) if i % 2 else bytes(4)
        seq = int(rng.integers(0, 1 << 63)) * 2 + (i & 1) if i % 3 else (1 << 64) - 1 - i
        frames.append((key, salt, seq, aad, bytes(rng.integers(0, 256, l, dtype=np.uint8))))
    plain, sealed, rec = bytearray(), bytearray(), []
    for key, salt, seq, aad, f in frames:
        a = min(aad, len(f))
        ct, tag = ssl.seal(key, ac.nonce_of(salt, seq), f[:a], f[a:])
        rec.append((key, salt, seq, aad, len(f), len(plain), tag))
        plain += ac.pad16(f)
        sealed += ac.pad16(f[:a] + ct)
    edges = ac.poly_edges()
    msg, prec = bytearray(), []
    for _, otk, m in edges:
        prec.append((otk, len(m), len(msg), ssl.poly1305(otk, m)))
        msg += ac.pad16(m)
    u8 = lambda rows: np.array([np.frombuffer(r, np.uint8) for r in rows], dtype=np.uint8)
    os.makedirs(os.path.join(HERE, "aead"), exist_ok=True)
    np.savez_compressed(
        os.path.join(HERE, "aead", "aead_vectors.npz"),
        key=u8([r[0] for r in rec]), salt=u8([r[1] for r in rec]), seq=np.array([r[2] for r in rec], dtype=np.uint64),
        aad=np.array([r[3] for r in rec], dtype=np.uint32), len=np.array([r[4] for r in rec], dtype=np.uint32),
        start=np.array([r[5] for r in rec], dtype=np.uint32), tag=u8([r[6] for r in rec]),
        plain=np.frombuffer(bytes(plain), np.uint8), sealed=np.frombuffer(bytes(sealed), np.uint8),
        otk=u8([r[0] for r in prec]), mlen=np.array([r[1] for r in prec], dtype=np.uint32),
        mstart=np.array([r[2] for r in prec], dtype=np.uint32), ptag=u8([r[3] for r in prec]),
        msg=np.frombuffer(bytes(msg), np.uint8))
    print(f"{len(rec)} frames, {len(prec)} Poly1305 messages")


if __name__ == "__main__":
    main()
