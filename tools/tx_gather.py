#!/usr/bin/env python3
"""Time the tx gather (cop_tx_gather, cop_submit_tx) against a plain copy.

Workloads: 32 batches of 65,536 64-byte frames (fw1k rules) with the
generator's default traffic (about two thirds forwarded) and with its drop
classes turned down (about 94 % forwarded), and 32 IMIX batches of 65,536
frames; the forwarded share is reported. Per workload:
  gather      cop_tx_gather of lists that exist already, to the return of cop_sync
  submit      cop_submit alone
  submit_tx   cop_submit_tx (pipeline + gather on one lane)
  d2d         cop_memcpy_d2d of as many bytes as the gather wrote (the yardstick:
              a contiguous copy)
each the median (min-max) of --runs host wall-clock runs after --warmup.
The gather's traffic is what it reads plus what it writes (frames twice, list
words, off / len words). One JSON line per workload.

  python tools/tx_gather.py [--batches 32] [--n 65536] [--runs 15] [--warmup 3] [--once]

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


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def workload(ctx, name, nb, n, rules, opts, imix, runs, warmup):
    batches, txs, keep = [], [], []
    out_bytes = 0
    for b in range(nb):
        if imix:
            slab, offs = cg.gen_imix(0x7A000 + b, n, rules, None, opts)
            lens = np.minimum(np.diff(np.append(offs.astype(np.int64), len(slab) - 64)), cg.TX_MAX_FRAME)
            lens = np.maximum(lens, 1).astype(np.uint32)
            dp, do, dl = ctx.alloc(slab.nbytes), ctx.alloc(n * 4), ctx.alloc(n * 4)
            dp.upload(slab)
            do.upload(offs)
            dl.upload(lens)
            cap = int(((lens.astype(np.int64) + 15) & ~15).sum()) + 64
        else:
            pk = cg.gen_trace(0x7A000 + b, n, rules, None, 64, opts)
            dp, do, dl = ctx.alloc(pk.nbytes), None, None
            dp.upload(pk)
            cap = n * 64
        dr, df, dc = ctx.alloc(n * 8), ctx.alloc(n * 4), ctx.alloc(16)
        fr, off, ln, st = ctx.alloc(cap), ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(16)
        batches.append(cg.make_batch(dp, n, dr, 64, offsets=do, fwd_idx=df, fwd_count=dc))
        txs.append(cg.make_tx(dict(frames=fr, off=off, len=ln, status=st, cap_bytes=cap, cap_frames=n), lens=dl,
                              copy_bytes=0 if imix else 64))
        keep.append((dp, do, dl, dr, df, dc, fr, off, ln, st))

    def submit():
        ctx.submit(batches)
        ctx.sync()

    def submit_tx():
        ctx.submit_tx(batches, txs)
        ctx.sync()

    def gather():
        ctx.tx_gather(batches, txs)
        ctx.sync()

    submit_tx()
    frames = used = 0
    for k in keep:
        s = k[9].download(np.uint32, 4)
        assert s[2] == 0, "a burst overflowed"
        frames += int(s[0])
        used += int(s[1])
    src, dst = ctx.alloc(max(used, 16)), ctx.alloc(max(used, 16))

    def d2d():
        cg._check(cg.lib().cop_memcpy_d2d(ctx.handle, dst.ptr, src.ptr, used), ctx, "d2d")
        ctx.sync()

    res = {"workload": name, "batches": nb, "n": n, "forwarded": round(frames / (nb * n), 4), "frames": frames,
           "out_bytes": used, "traffic_bytes": 2 * used + 12 * frames}
    for key, fn in (("gather", gather), ("submit", submit), ("submit_tx", submit_tx), ("d2d", d2d)):
        res[key] = timed(fn, runs, warmup)
    g, d = res["gather"]["median_us"], res["d2d"]["median_us"]
    res["gather_GBps"] = round(res["traffic_bytes"] / g / 1e3, 1)
    res["d2d_GBps"] = round(2 * used / d / 1e3, 1)
    res["gather_over_d2d"] = round(g / d, 2)
    res["submit_tx_minus_submit_us"] = round(res["submit_tx"]["median_us"] - res["submit"]["median_us"], 1)
    return res


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
    rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    half = None
    most = cg.trace_opts(pct_non_ipv4=0, pct_bad_version=0, pct_unknown_dst=0, pct_src_in_rule=4)
    for name, opts, imix in (("slot64_half", half, False), ("slot64_most", most, False), ("imix", most, True)):
        with cg.Context(stages=cg.STAGE_PARSE | cg.STAGE_FW, max_batch=a.n, max_batches=a.batches) as ctx:
            ctx.set_fw_table(cg.LpmTable(rules, 1024, 24))
            print(json.dumps(workload(ctx, name, a.batches, a.n, rules, opts, imix, a.runs, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
