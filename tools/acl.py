#!/usr/bin/env python3
"""Time cop_acl_filter and cop_acl_classify against cop_sketch_police and cop_fwd_check over the same lists.

Workload: 32 batches of 65,536 frames of the fw1k trace (64-byte slots, then
IMIX), every IPv4 header option-less with a valid checksum, the forward lists
the pipeline's. Rule sets of 128 and 1,024 generated rules: source prefixes
around addresses the trace carries (depths 8..32), half of them with a
destination prefix, port ranges and protocols on some, priorities 0..15, a
third of them dropping, and a lowest-priority permit-all. Per workload and
rule set:
  filter      cop_acl_filter of the pipeline's lists (COP_ACL_COUNTERS)
  filter_nc   the same on an ACL without counters
  classify    cop_acl_classify of every packet
  police      cop_sketch_police of the same lists (a yardstick: the same grid and two-kernel shape)
  check       cop_fwd_check of the same lists, 1,024-entry table (the other yardstick)
each the median (min-max) of --runs host wall-clock runs after --warmup, to
the return of cop_sync. One JSON line per workload and rule set.

  python tools/acl.py [--batches 32] [--n 65536] [--rules 128,1024] [--runs 15] [--warmup 3] [--once]

--once: a single pass per call (for a rocprofv3 --kernel-trace --stats or --pmc run).
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


def l3_headers(pk, starts):
    """Option-less headers, no fragments, TTL 64 and valid checksums at the IPv4 frames that start at `starts`."""
    s = starts[(pk[starts + 12] == 8) & (pk[starts + 13] == 0) & ((pk[starts + 14] >> 4) == 4)]
    pk[s + 14] = 0x45
    pk[s + 20] = pk[s + 21] = 0
    pk[s + 22] = 64
    pk[s + 24] = pk[s + 25] = 0
    w = sum((pk[s + 14 + 2 * j].astype(np.int64) << 8) | pk[s + 15 + 2 * j] for j in range(10))
    for _ in range(3):
        w = (w & 0xFFFF) + (w >> 16)
    hc = ~w & 0xFFFF
    pk[s + 24], pk[s + 25] = hc >> 8, hc & 0xFF
    return s


def be32(pk, s, o):
    return sum(pk[s + o + j].astype(np.uint64) << np.uint64(24 - 8 * j) for j in range(4))


def gen_acl_rules(n, src, dst, seed=0xAC1):
    rng = np.random.default_rng(seed + n)
    r = cg.acl_rules(n)
    r["src_ip"] = src[rng.integers(0, len(src), n)]
    r["src_depth"] = np.array([8, 16, 20, 24, 28, 32])[rng.integers(0, 6, n)]
    r["dst_ip"] = dst[rng.integers(0, len(dst), n)]
    r["dst_depth"] = np.array([0, 0, 0, 8, 16, 24])[rng.integers(0, 6, n)]
    u = rng.random(n)
    r["dport_hi"] = np.where(u < 0.4, 1023, 0xFFFF)
    one = (u >= 0.4) & (u < 0.5)
    port = rng.integers(0, 65536, n)
    r["dport_lo"], r["dport_hi"] = np.where(one, port, 0), np.where(one, port, r["dport_hi"])
    r["proto"] = np.where(rng.random(n) < 0.5, 6, 17)
    r["proto_mask"] = np.where(rng.random(n) < 0.5, 0xFF, 0)
    r["priority"] = rng.integers(0, 16, n)
    r["action"] = rng.integers(0, 3, n) == 0
    r[n - 1] = cg.acl_rules(1)[0]
    r["priority"][n - 1] = -1
    return r


def workload(ctx, name, nb, n, fw_rules, opts, imix, rule_counts, runs, warmup):
    rng = np.random.default_rng(0xAC7)
    batches, descs, pols, checks, keep = [], [], [], [], []
    src = dst = None
    for b in range(nb):
        if imix:
            pk, offs = cg.gen_imix(0x7A000 + b, n, fw_rules, None, opts)
            lens = np.minimum(np.diff(np.append(offs.astype(np.int64), len(pk) - 64)), cg.TX_MAX_FRAME)
            lens = np.maximum(lens, 1).astype(np.uint32)
            s = l3_headers(pk, offs.astype(np.int64)[lens >= 34])
            dp, do, dl = ctx.alloc(pk.nbytes), ctx.alloc(n * 4), ctx.alloc(n * 4)
            do.upload(offs)
            dl.upload(lens)
        else:
            pk = cg.gen_trace(0x7A000 + b, n, fw_rules, None, 64, opts)
            s = l3_headers(pk, np.arange(n, dtype=np.int64) * 64)
            dp, do, dl = ctx.alloc(pk.nbytes), None, None
        if src is None:
            src, dst = be32(pk, s[:4096], 26), be32(pk, s[:4096], 30)
        dp.upload(pk)
        dr, df, dc = ctx.alloc(n * 8), ctx.alloc(n * 4), ctx.alloc(16)
        w, oi, oc, st = ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(16), ctx.alloc(16)
        batches.append(cg.make_batch(dp, n, dr, 64, offsets=do, fwd_idx=df, fwd_count=dc))
        descs.append(cg.make_acl_desc(w, oi, oc, st))
        pols.append(cg.make_police(1 << 62, oi, oc, st))   # keeps everything: the lookups and every write
        checks.append(cg.make_fwd_check(oi, oc, st, lens=dl))
        keep.append((dr, st))
    ctx.submit(batches)
    ctx.sync()
    for dr, _ in keep:                       # every record a route hit on a random next hop
        rec = dr.download(cg.RESULT_DT, n)
        rec["flags"] |= cg.FLAG_ROUTE_HIT
        rec["route_nh"] = rng.integers(0, 1024, n)
        dr.upload(rec)
    status = lambda: np.array([k[1].download(np.uint32, 4) for k in keep])

    sk = ctx.sketch(4, 14, cg.SKETCH_KEY_SRC, 32, seed=1)
    sk.update(batches, 1 << cg.FORWARD)
    table = np.zeros(1024, dtype=cg.NEIGH_DT)
    table.view(np.uint8)[:] = rng.integers(0, 256, table.nbytes, dtype=np.uint8)
    table["flags"] = np.arange(1024) % 16 != 7
    ng = ctx.neigh(1024)
    ng.set(0, table)
    cfg = cg.fwd_config(cg.FWD_VERIFY_CSUM, 0)

    def police():
        sk.police(batches, pols)
        ctx.sync()

    def check():
        ctx.fwd_check(ng, cfg, batches, checks)
        ctx.sync()

    police()
    pst = status()
    check()
    cst = status()
    yard = {"police": timed(police, runs, warmup), "check": timed(check, runs, warmup)}
    out = []
    for nr in rule_counts:
        rules = gen_acl_rules(nr, src, dst)
        table_ = cg.AclTable(rules)
        acl, acl_nc = ctx.acl(table_, cg.ACL_COUNTERS), ctx.acl(table_)

        def flt(a=acl):
            a.filter(batches, descs)
            ctx.sync()

        def flt_nc():
            flt(acl_nc)

        def classify():
            acl.classify(batches, descs)
            ctx.sync()

        flt()
        ast = status()
        rep = table_.report
        res = {"workload": name, "batches": nb, "n": n, "n_rules": nr, "row_words": rep.row_words,
               "intervals": list(rep.n_intervals), "image_bytes": rep.image_bytes,
               "listed": int(ast[:, :2].sum()), "kept": int(ast[:, 0].sum()), "removed": int(ast[:, 1].sum()),
               "kept_miss": int(ast[:, 2].sum()), "kept_skip": int(ast[:, 3].sum()),
               "police_kept": int(pst[:, 0].sum()), "check_kept": int(cst[:, 0].sum())}
        for key, fn in (("filter", flt), ("filter_nc", flt_nc), ("classify", classify)):
            res[key] = timed(fn, runs, warmup)
        res.update(yard)
        res["filter_over_police"] = round(res["filter"]["median_us"] / yard["police"]["median_us"], 2)
        res["filter_over_check"] = round(res["filter"]["median_us"] / yard["check"]["median_us"], 2)
        hits = acl.counters()
        res["counted"] = int(hits.sum())
        res["top_rule_share"] = round(float(hits.max()) / max(int(hits.sum()), 1), 3)
        acl.destroy()
        acl_nc.destroy()
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--rules", default="128,1024")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.once:
        a.runs, a.warmup = 1, 0
    fw_rules = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    most = cg.trace_opts(pct_non_ipv4=0, pct_bad_version=0, pct_unknown_dst=0, pct_src_in_rule=4)
    for name, imix in (("slot64", False), ("imix", True)):
        with cg.Context(stages=cg.STAGE_PARSE | cg.STAGE_FW, max_batch=a.n, max_batches=a.batches) as ctx:
            ctx.set_fw_table(cg.LpmTable(fw_rules, 1024, 24))
            for res in workload(ctx, name, a.batches, a.n, fw_rules, most, imix, [int(x) for x in a.rules.split(",")],
                                a.runs, a.warmup):
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
