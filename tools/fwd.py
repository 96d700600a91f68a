#!/usr/bin/env python3
"""Time cop_fwd_check and cop_fwd_rewrite against cop_tx_gather of the same frames.

Workload: 32 batches of 65,536 frames of the fw1k trace (64-byte slots, then
IMIX), every IPv4 header option-less with a valid checksum and a TTL of 32..255
(1 in 128: TTL 1), the forward lists the pipeline's, every record a route hit
on a uniformly random next hop of a 1 << 20 entry neighbour table (16 MiB; --entries
for another size) of which 15 in 16 entries are valid. Per workload:
  check       cop_fwd_check of the pipeline's lists (COP_FWD_VERIFY_CSUM, with exception lists)
  gather      cop_tx_gather of the check's lists (the yardstick)
  rewrite     cop_fwd_rewrite of the gathered bursts (with port[])
  chain       check, gather, rewrite queued without a sync between them
  host        cop_fwd_check_host + cop_fwd_rewrite_host over the same arrays in host memory (--host-runs)
each the median (min-max) of --runs host wall-clock runs after --warmup, to
the return of cop_sync. The rewrite decrements in place, so a frame's TTL falls
by one per run; 32 and above stays forwardable for every run. One JSON line
per workload.

  python tools/fwd.py [--batches 32] [--n 65536] [--entries 1048576] [--runs 15] [--warmup 3] [--host-runs 3] [--once]

--entries 1024: the table stays in L2, so what the scattered 16-byte entry loads cost shows in the difference.
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


def l3_headers(pk, starts, rng):
    """Option-less headers, TTLs and valid checksums at the IPv4 frames that start at `starts`."""
    s = starts[(pk[starts + 12] == 8) & (pk[starts + 13] == 0) & ((pk[starts + 14] >> 4) == 4)]
    pk[s + 14] = 0x45
    ttl = rng.integers(32, 256, len(s))
    ttl[rng.integers(0, 128, len(s)) == 0] = 1
    pk[s + 22] = ttl
    pk[s + 24] = pk[s + 25] = 0
    w = sum((pk[s + 14 + 2 * j].astype(np.int64) << 8) | pk[s + 15 + 2 * j] for j in range(10))
    for _ in range(3):
        w = (w & 0xFFFF) + (w >> 16)
    hc = ~w & 0xFFFF
    pk[s + 24], pk[s + 25] = hc >> 8, hc & 0xFF


def aligned(nbytes, fill=0):
    raw = np.full(nbytes + 64, fill, dtype=np.uint8)
    o = (-raw.ctypes.data) % 64
    return raw[o:o + nbytes]


def workload(ctx, ng, table, name, nb, n, rules, opts, imix, runs, warmup, host_runs):
    N_ENTRIES = len(table)
    rng = np.random.default_rng(0xF3D)
    cfg = cg.fwd_config(cg.FWD_VERIFY_CSUM, 0)
    batches, checks, filtered, txs, rws, keep, host = [], [], [], [], [], [], []
    for b in range(nb):
        if imix:
            pk, offs = cg.gen_imix(0x7A000 + b, n, rules, None, opts)
            lens = np.minimum(np.diff(np.append(offs.astype(np.int64), len(pk) - 64)), cg.TX_MAX_FRAME)
            lens = np.maximum(lens, 1).astype(np.uint32)
            l3_headers(pk, offs.astype(np.int64)[lens >= 34], rng)
            dp, do, dl = ctx.alloc(pk.nbytes), ctx.alloc(n * 4), ctx.alloc(n * 4)
            do.upload(offs)
            dl.upload(lens)
            cap = int(((lens.astype(np.int64) + 15) & ~15).sum()) + 64
        else:
            pk = cg.gen_trace(0x7A000 + b, n, rules, None, 64, opts)
            l3_headers(pk, np.arange(n, dtype=np.int64) * 64, rng)
            offs = lens = None
            dp, do, dl = ctx.alloc(pk.nbytes), None, None
            cap = n * 64
        dp.upload(pk)
        dr, df, dc = ctx.alloc(n * 8), ctx.alloc(n * 4), ctx.alloc(16)
        oi, oc, ei, ec, cs = ctx.alloc(n * 4), ctx.alloc(16), ctx.alloc(n * 4), ctx.alloc(16), ctx.alloc(16)
        fr, off, ln, st, port, rs = ctx.alloc(cap), ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(16), ctx.alloc(n * 4), ctx.alloc(16)
        batches.append(cg.make_batch(dp, n, dr, 64, offsets=do, fwd_idx=df, fwd_count=dc))
        checks.append(cg.make_fwd_check(oi, oc, cs, lens=dl, exc_idx=ei, exc_count=ec))
        filtered.append(cg.make_batch(dp, n, dr, 64, offsets=do, fwd_idx=oi, fwd_count=oc))
        txs.append(cg.make_tx(dict(frames=fr, off=off, len=ln, status=st, cap_bytes=cap, cap_frames=n), lens=dl,
                              copy_bytes=0 if imix else 64))
        rws.append(cg.make_fwd_rw(rs, port))
        keep.append((dr, df, dc, cs, st, rs))
        host.append((pk, offs, lens, cap))
    ctx.submit(batches)
    ctx.sync()
    recs = []
    for dr, *_ in keep:                      # every record a route hit on a random next hop
        rec = dr.download(cg.RESULT_DT, n)
        rec["flags"] |= cg.FLAG_ROUTE_HIT
        rec["route_nh"] = rng.integers(0, N_ENTRIES, n)
        dr.upload(rec)
        recs.append(rec)

    def check():
        ctx.fwd_check(ng, cfg, batches, checks)
        ctx.sync()

    def gather():
        ctx.tx_gather(filtered, txs)
        ctx.sync()

    def rewrite():
        ctx.fwd_rewrite(ng, cfg, filtered, txs, rws)
        ctx.sync()

    def chain():
        ctx.fwd_check(ng, cfg, batches, checks)
        ctx.tx_gather(filtered, txs)
        ctx.fwd_rewrite(ng, cfg, filtered, txs, rws)
        ctx.sync()

    chain()
    cst = np.array([k[3].download(np.uint32, 4) for k in keep])
    txst = np.array([k[4].download(np.uint32, 4) for k in keep])
    rwst = np.array([k[5].download(np.uint32, 4) for k in keep])
    assert (txst[:, 2] == 0).all(), "a burst overflowed"
    res = {"workload": name, "batches": nb, "n": n, "n_entries": N_ENTRIES,
           "listed": int(cst[:, :2].sum()), "kept": int(cst[:, 0].sum()), "removed_ttl": int(cst[:, 2].sum()),
           "removed_no_neigh": int(cst[:, 3].sum()), "frames": int(txst[:, 0].sum()), "out_bytes": int(txst[:, 1].sum()),
           "rewritten": int(rwst[:, 0].sum()), "pass": int(rwst[:, 1].sum())}
    for key, fn in (("check", check), ("gather", gather), ("rewrite", rewrite), ("chain", chain)):
        res[key] = timed(fn, runs, warmup)
    res["check_over_gather"] = round(res["check"]["median_us"] / res["gather"]["median_us"], 2)
    res["rewrite_over_gather"] = round(res["rewrite"]["median_us"] / res["gather"]["median_us"], 2)

    # the host mirror over the same arrays
    hb, hc, hf, ht, hr, hold = [], [], [], [], [], []
    for (pk, offs, lens, cap), (dr, df, dc, *_), rec in zip(host, keep, recs):
        a = {"pk": aligned(pk.nbytes), "res": aligned(n * 8), "idx": aligned(n * 4), "cnt": aligned(16), "oi": aligned(n * 4),
             "oc": aligned(16), "cs": aligned(16), "fr": aligned(cap), "off": aligned(n * 4), "ln": aligned(n * 4),
             "st": aligned(16), "port": aligned(n * 4), "rs": aligned(16)}
        a["pk"][:], a["res"][:] = pk, rec.view(np.uint8)
        a["idx"][:], a["cnt"][:] = df.download(np.uint8, n * 4), dc.download(np.uint8, 16)
        p = {k: v.ctypes.data for k, v in a.items()}
        o_, l_ = (offs.ctypes.data, lens.ctypes.data) if imix else (None, None)
        hb.append(cg.make_batch(p["pk"], n, p["res"], 64, offsets=o_, fwd_idx=p["idx"], fwd_count=p["cnt"]))
        hc.append(cg.make_fwd_check(p["oi"], p["oc"], p["cs"], lens=l_))
        hf.append(cg.make_batch(p["pk"], n, p["res"], 64, offsets=o_, fwd_idx=p["oi"], fwd_count=p["oc"]))
        ht.append(cg.make_tx(dict(frames=p["fr"], off=p["off"], len=p["ln"], status=p["st"], cap_bytes=cap, cap_frames=n),
                             lens=l_, copy_bytes=0 if imix else 64))
        hr.append(cg.make_fwd_rw(p["rs"], p["port"]))
        hold.append(a)

    def host_check():
        assert cg.fwd_check_host(table, cfg, hb, hc) == 0

    def host_rewrite():
        assert cg.fwd_rewrite_host(table, cfg, hf, ht, hr) == 0

    host_check()
    assert cg.tx_gather_host(hf, ht) == 0
    res["host_check"] = timed(host_check, host_runs, 0)
    res["host_rewrite"] = timed(host_rewrite, host_runs, 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--entries", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.once:
        a.runs, a.warmup, a.host_runs = 1, 0, 1
    rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    most = cg.trace_opts(pct_non_ipv4=0, pct_bad_version=0, pct_unknown_dst=0, pct_src_in_rule=4)
    rng = np.random.default_rng(0x7AB1E)
    N_ENTRIES = a.entries
    table = np.zeros(N_ENTRIES, dtype=cg.NEIGH_DT)
    table.view(np.uint8)[:] = rng.integers(0, 256, table.nbytes, dtype=np.uint8)
    table["flags"] = np.arange(N_ENTRIES) % 16 != 7
    table["port"] %= 8
    for name, imix in (("slot64", False), ("imix", True)):
        with cg.Context(stages=cg.STAGE_PARSE | cg.STAGE_FW, max_batch=a.n, max_batches=a.batches) as ctx:
            ctx.set_fw_table(cg.LpmTable(rules, 1024, 24))
            ng = ctx.neigh(N_ENTRIES)
            ng.set(0, table)
            print(json.dumps(workload(ctx, ng, table, name, a.batches, a.n, rules, most, imix, a.runs, a.warmup,
                                      a.host_runs)), flush=True)


if __name__ == "__main__":
    main()
