#!/usr/bin/env python3
"""Time the sketch calls (cop_sketch_update / police / query) against cop_submit.

Workload: 32 batches of 65,536 64-byte frames of the fw1k trace. Per sketch
size (4 x 2^14 and 4 x 2^20 columns) and source kind (the generator's sources,
uniformly random sources, one single source):
  update      cop_sketch_update of every packet (verdict_mask 0), to the return of cop_sync
and once, on the generator's sources:
  submit      cop_submit of the same batches (the yardstick: it reads the same header bytes)
  police      cop_sketch_police of the lists cop_submit wrote, threshold = the median estimate
  query       cop_sketch_query of 2M addresses
each the median (min-max) of --runs host wall-clock runs after --warmup. An
update issues rows atomics per counting packet before combining; the implied
rate is counting * rows / time. One JSON line per measurement.

  python tools/sketch.py [--batches 32] [--n 65536] [--runs 15] [--warmup 3] [--combine 1] [--once]

--combine 0: equal keys are not combined before going to memory (timing A/B:
the single-source against uniform ratio is what the combine is for).
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

ROWS = 4


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def traces(nb, n, rules, kind):
    """nb traces of n 64-byte frames; (frames, packets that count as IPv4)."""
    out, counting = [], 0
    rng = np.random.default_rng(0x5CE7)
    for b in range(nb):
        pk = cg.gen_trace(0x7A000 + b, n, rules, None, 64, None)
        f = pk.reshape(n, 64)
        if kind == "uniform":
            f[:, 26:30] = rng.integers(0, 256, (n, 4), dtype=np.uint8)
        elif kind == "single":
            f[:, 26:30] = (10, 1, 2, 3)
        counting += int(((f[:, 12] == 8) & (f[:, 13] == 0) & ((f[:, 14] >> 4) == 4)).sum())
        out.append(pk)
    return out, counting


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--combine", type=int, default=1)
    ap.add_argument("--queries", type=int, default=1 << 21)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.once:
        a.runs, a.warmup = 1, 0
    os.environ["COP_SKETCH_COMBINE"] = str(a.combine)     # read by the library at its first update
    rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    nb, n = a.batches, a.n
    with cg.Context(stages=cg.STAGE_PARSE | cg.STAGE_FW, max_batch=n, max_batches=nb) as ctx:
        ctx.set_fw_table(cg.LpmTable(rules, 1024, 24))
        bufs = [(ctx.alloc(n * 64), ctx.alloc(n * 8), ctx.alloc(n * 4), ctx.alloc(16)) for _ in range(nb)]
        batches = [cg.make_batch(dp, n, dr, 64, fwd_idx=df, fwd_count=dc) for dp, dr, df, dc in bufs]
        base = {"batches": nb, "n": n, "rows": ROWS, "combine": a.combine}
        for kind in ("gen", "uniform", "single"):
            pks, counting = traces(nb, n, rules, kind)
            for (dp, _, _, _), pk in zip(bufs, pks):
                dp.upload(pk)
            for lc in (14, 20):
                sk = ctx.sketch(ROWS, lc, cg.SKETCH_KEY_SRC, 32, seed=1)

                def update():
                    sk.update(batches, 0)
                    ctx.sync()

                r = dict(base, call="update", sources=kind, log2_cols=lc, counter_bytes=8 * ROWS << lc, counting=counting,
                         **timed(update, a.runs, a.warmup))
                r["atomics_per_s_before_combining"] = round(counting * ROWS / r["median_us"] * 1e6)
                print(json.dumps(r), flush=True)
                sk.destroy()
        # the yardstick, police and query on the generator's sources
        pks, counting = traces(nb, n, rules, "gen")
        for (dp, _, _, _), pk in zip(bufs, pks):
            dp.upload(pk)

        def submit():
            ctx.submit(batches)
            ctx.sync()

        print(json.dumps(dict(base, call="submit", sources="gen", **timed(submit, a.runs, a.warmup))), flush=True)
        for lc in (14, 20):
            sk = ctx.sketch(ROWS, lc, cg.SKETCH_KEY_SRC, 32, seed=1)
            sk.update(batches, 0)
            ips = np.ascontiguousarray(np.concatenate([p.reshape(n, 64)[:, 26:30] for p in pks]))
            ips = ips.view(">u4").astype(np.uint32).ravel()
            ips = np.resize(ips, a.queries)
            d_ips, d_est = ctx.alloc(4 * a.queries), ctx.alloc(8 * a.queries)
            d_ips.upload(ips)

            def query():
                sk.query(d_ips, a.queries, d_est)
                ctx.sync()

            r = dict(base, call="query", sources="gen", log2_cols=lc, addresses=a.queries, **timed(query, a.runs, a.warmup))
            r["gathers_per_s"] = round(a.queries * ROWS / r["median_us"] * 1e6)
            print(json.dumps(r), flush=True)
            th = int(np.median(d_est.download(np.uint64, a.queries)))
            outs = [(ctx.alloc(n * 4), ctx.alloc(16), ctx.alloc(16)) for _ in range(nb)]
            pol = [cg.make_police(th, *o) for o in outs]

            def police():
                sk.police(batches, pol)
                ctx.sync()

            r = dict(base, call="police", sources="gen", log2_cols=lc, threshold=th, **timed(police, a.runs, a.warmup))
            st = np.array([o[2].download(np.uint32, 4) for o in outs])
            r["kept"], r["removed"] = int(st[:, 0].sum()), int(st[:, 1].sum())
            print(json.dumps(r), flush=True)
            sk.destroy()


if __name__ == "__main__":
    main()
