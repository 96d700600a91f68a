#!/usr/bin/env python3
"""Time cop_aead_seal / cop_aead_open against cop_tx_gather of the same frames.

Workloads, --batches bursts of --n frames each, aad_bytes 34:
  slot    64-byte frames at 64-byte slots
  imix    64 / 594 / 1518-byte frames 7 : 4 : 1 in a shuffled order, off / len form
Per workload:
  seal, open   host wall clock to the return of cop_sync
  gather       cop_tx_gather of the same frames through identity forward lists (the yardstick: it
               moves the same bytes, so seal / gather says how far from memory-bound the cipher is)
  host         cop_aead_seal_host of one burst on one core
each the median (min-max) of --runs runs after --warmup. Gbit/s counts the frames' own bytes; a
ChaCha block is counted per 64 bytes of text or part of them plus one per frame for the one-time
key, at OPS_PER_BLOCK 32-bit integer operations (80 quarter rounds of 4 adds, 4 xors and 4
rotates, and the 16 final adds). One JSON line per measurement.

  python tools/aead.py [--batches 32] [--n 65536] [--runs 15] [--warmup 3] [--once]

--once: a single pass per call (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ghost-dataplane_amd"))
import copgpu as cg  # noqa: E402

AAD = 34
OPS_PER_BLOCK = 80 * 12 + 16
# 256 CUs x 4 SIMDs x 32 lanes per clock x 2.4 GHz: one 32-bit integer operation per lane and clock
PEAK_INT_OPS = 256 * 4 * 32 * 2.4e9


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def rates(r, frame_bytes, blocks):
    s = r["median_us"] * 1e-6
    r["gbit_per_s"] = round(frame_bytes * 8 / s / 1e9, 1)
    r["chacha_blocks_per_s"] = round(blocks / s)
    r["int_ops_per_s"] = round(blocks * OPS_PER_BLOCK / s)
    r["share_of_int_peak"] = round(blocks * OPS_PER_BLOCK / s / PEAK_INT_OPS, 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.once:
        a.runs, a.warmup = 1, 0
    nb, n = a.batches, a.n
    rng = np.random.default_rng(0xAEAD)
    key = cg.aead_key(bytes(rng.integers(0, 256, 32, dtype=np.uint8)))
    with cg.Context(stages=cg.STAGE_PARSE, max_batch=n, max_batches=nb) as ctx:
        for kind in ("slot", "imix"):
            if kind == "slot":
                lens = np.full(n, 64, dtype=np.uint32)
            else:
                lens = rng.permutation(np.resize(np.array([64] * 7 + [594] * 4 + [1518], dtype=np.uint32), n))
            ext = (lens.astype(np.int64) + 15) & ~15
            off = (np.cumsum(ext) - ext).astype(np.uint32)
            cap = int(ext.sum())
            frame_bytes = int(lens.sum()) * nb
            blocks = int((1 + (lens.astype(np.int64) - AAD + 63) // 64).sum()) * nb
            src = rng.integers(0, 256, cap, dtype=np.uint8)
            idx = np.arange(n, dtype=np.uint32)
            bufs = []
            for _ in range(nb):
                d = {k: ctx.alloc(v) for k, v in (("src", cap), ("frames", cap), ("off", 4 * n), ("len", 4 * n),
                                                  ("tags", 16 * n), ("ok", 4 * n), ("status", 16), ("gstatus", 16),
                                                  ("idx", 4 * n), ("cnt", 16), ("goff", 4 * n), ("glen", 4 * n))}
                d["src"].upload(src)
                d["frames"].upload(src)
                d["off"].upload(off)
                d["len"].upload(lens)
                d["idx"].upload(idx)
                d["cnt"].upload(np.array([n, 0, 0, 0], dtype=np.uint32))
                bufs.append(d)

            def bursts(with_ok):
                if kind == "slot":
                    return [cg.make_aead_burst(d["frames"], d["tags"], d["status"], n, cap, ok=d["ok"] if with_ok else None,
                                               seq_base=i * n, slot_bytes=64, frame_bytes=64, aad_bytes=AAD)
                            for i, d in enumerate(bufs)]
                return [cg.make_aead_burst(d["frames"], d["tags"], d["status"], n, cap, off=d["off"], len=d["len"],
                                           ok=d["ok"] if with_ok else None, seq_base=i * n, aad_bytes=AAD)
                        for i, d in enumerate(bufs)]

            sb, ob = bursts(False), bursts(True)
            if kind == "slot":
                batches = [cg.make_batch(d["src"], n, None, 64, fwd_idx=d["idx"], fwd_count=d["cnt"]) for d in bufs]
                tx = [cg.make_tx((d["frames"], d["goff"], d["glen"], d["gstatus"], cap, n), copy_bytes=64) for d in bufs]
            else:
                batches = [cg.make_batch(d["src"], n, None, 0, offsets=d["off"], fwd_idx=d["idx"], fwd_count=d["cnt"])
                           for d in bufs]
                tx = [cg.make_tx((d["frames"], d["goff"], d["glen"], d["gstatus"], cap, n), lens=d["len"]) for d in bufs]

            def gather():
                ctx.tx_gather(batches, tx)
                ctx.sync()

            def seal():
                ctx.aead_seal(key, sb)
                ctx.sync()

            def open_():
                ctx.aead_open(key, ob)
                ctx.sync()

            base = {"workload": kind, "bursts": nb, "n": n, "aad_bytes": AAD, "frame_bytes": frame_bytes}
            g = dict(base, call="gather", **timed(gather, a.runs, a.warmup))
            g["gbit_per_s"] = round(frame_bytes * 8 / (g["median_us"] * 1e-6) / 1e9, 1)
            print(json.dumps(g), flush=True)
            # seal and open alternate so that every open sees sealed frames: time them in pairs
            ts, to = [], []
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                seal()
                t1 = time.perf_counter()
                open_()
                t2 = time.perf_counter()
                if i >= a.warmup:
                    ts.append((t1 - t0) * 1e6)
                    to.append((t2 - t1) * 1e6)
            for call, t in (("seal", ts), ("open", to)):
                r = dict(base, call=call, median_us=round(float(np.median(t)), 1), min_us=round(min(t), 1),
                         max_us=round(max(t), 1), chacha_blocks=blocks)
                r = rates(r, frame_bytes, blocks)
                r["times_gather"] = round(r["median_us"] / g["median_us"], 2)
                print(json.dumps(r), flush=True)
            st = np.array([d["status"].download(np.uint32, 4) for d in bufs])
            assert (st[:, 0] == n).all() and (st[:, 1:] == 0).all(), st[:4]       # every frame opened, none forged
            assert np.array_equal(bufs[0]["frames"].download(np.uint8, cap), src)
            # the host mirror, one burst on one core
            def aligned(nbytes):
                raw = np.zeros(nbytes + 64, dtype=np.uint8)
                o = (-raw.ctypes.data) % 64
                return raw[o:o + nbytes]

            hf, ht, hs = aligned(cap), aligned(16 * n), aligned(16).view(np.uint32)
            hf[:] = src
            hb = cg.make_aead_burst(hf.ctypes.data, ht.ctypes.data, hs.ctypes.data, n, cap,
                                    off=None if kind == "slot" else off.ctypes.data,
                                    len=None if kind == "slot" else lens.ctypes.data, seq_base=0,
                                    slot_bytes=64 if kind == "slot" else 0, frame_bytes=64 if kind == "slot" else 0,
                                    aad_bytes=AAD)
            h = dict(base, call="host_seal_one_burst_one_core", bursts=1, frame_bytes=frame_bytes // nb,
                     **timed(lambda: cg.aead_seal_host(key, [hb]), min(a.runs, 5), min(a.warmup, 1)))
            print(json.dumps(rates(h, frame_bytes // nb, blocks // nb)), flush=True)
            for d in bufs:
                for b in d.values():
                    b.free()


if __name__ == "__main__":
    main()
