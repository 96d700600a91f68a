#!/usr/bin/env python3
"""Time cop_lookup_bulk (rte_lpm_lookup_bulk on the device) per table form.

n = 2^24 device-resident addresses through one stage's table, timed with
cop_timer_start / cop_timer_stop around one call, median of 15 after 3
warm-up repetitions. Tables and forms: the 1000-rule firewall in LDS; 100k
routes in DIR-24-8 (plain and packed tbl8 groups), trie and bucketed form;
1M routes in DIR-24-8 and bucketed form. Two address sets each: uniform
random, and "in-table" (65 % inside a random prefix of the table, the rest
uniform). Prints one JSON line per case: Mlookup/s and GB/s at the 8
algorithmic bytes of a lookup (4 in, 4 out). The first lookups of every case
are compared with the host words.

--pipeline adds, for context, what was the only device route to the same
answers before: the one-shot FW | LPM pipeline over 64-byte frames carrying
the same addresses, on the same 100k table (fw1k as the firewall).

    python tools/lookup_bulk.py [--log2n 24] [--reps 15] [--warmup 3] [--pipeline] [--skip-1m]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ghost-dataplane_amd"))
import copgpu as cg  # noqa: E402

F, L = cg.STAGE_FW, cg.STAGE_LPM
DIR = cg.CFG_FW_FORCE_DIR24 | cg.CFG_LPM_FORCE_DIR24


_sets = {}


def address_sets(rules, n, seed):
    key = (id(rules), n, seed)
    if key not in _sets:
        _sets.clear()                     # one table's sets at a time (128 MiB)
        _sets[key] = make_sets(rules, n, seed)
    return _sets[key]


def make_sets(rules, n, seed):
    rng = np.random.default_rng(seed)
    uni = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    r = rules[rng.integers(0, len(rules), n)]
    span = (np.uint64(1) << (np.uint64(32) - r["depth"].astype(np.uint64))) - np.uint64(1)
    inside = (r["ip"].astype(np.uint64) & ~span & np.uint64(0xFFFFFFFF)) | (rng.integers(0, 1 << 32, n, dtype=np.uint64) & span)
    mix = np.where(rng.random(n) < 0.65, inside, rng.integers(0, 1 << 32, n, dtype=np.uint64)).astype(np.uint32)
    return {"uniform": uni, "in-table": mix}


def timed(ctx, fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        ctx.timer_start()
        fn()
        t = ctx.timer_stop()
        if i >= warmup:
            ms.append(t)
    return statistics.median(ms), min(ms), max(ms)


def case(name, stage, table, rules, flags, tbl8, want_form, a):
    os.environ["COP_TBL8"] = tbl8
    n = 1 << a.log2n
    with cg.Context(stages=F | L, flags=flags) as ctx:
        (ctx.set_fw_table if stage == F else ctx.set_route_lpm)(table)
        form = ctx.lookup_form(stage)
        assert want_form is None or form == want_form, (name, form, want_form)
        din, dout = ctx.alloc(n * 4), ctx.alloc(n * 4)
        for kind, ips in address_sets(rules, n, 0x100C0B).items():
            din.upload(ips)
            med, lo, hi = timed(ctx, lambda: ctx.lookup_bulk(stage, din, n, dout), a.reps, a.warmup)
            ctx.sync()
            k = min(n, 1 << 16)
            got = dout.download(np.uint32, k)
            want = table.lookup_words(ips[:k], cg.LOOKUP_RULE if stage == F else cg.LOOKUP_NH)
            assert np.array_equal(got, want), name
            print(json.dumps({"case": name, "form": form, "addresses": kind, "n": n, "median_ms": round(med, 4),
                              "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                              "mlookup_s": round(n / med / 1e3, 1), "gb_s": round(8 * n / med / 1e6, 1),
                              "hit_share": round(float(((want & cg.LOOKUP_HIT) != 0).mean()), 3)}), flush=True)


def pipeline(fw_rules, routes, rt, a):
    """The one-shot FW | LPM pipeline over frames carrying the in-table
    addresses as destinations (sources uniform): Mpkt/s for the same answers."""
    os.environ["COP_TBL8"] = "plain"
    B, nb = 262144, 16
    n = B * nb
    dst = address_sets(routes, n, 0x100C0B)["in-table"]
    src = address_sets(fw_rules, n, 0x100C0C)["uniform"]
    pk = cg.gen_trace(0x5EED0E00, n, None, None, opts=cg.trace_opts(pct_non_ipv4=0, pct_bad_version=0, pct_unknown_dst=0))
    f = pk.reshape(n, 64)
    f[:, 26:30] = src.astype(">u4").view(np.uint8).reshape(-1, 4)
    f[:, 30:34] = dst.astype(">u4").view(np.uint8).reshape(-1, 4)
    with cg.Context(stages=F | L, max_batch=B, max_batches=32, flags=cg.CFG_NO_COMPACT) as ctx:
        ctx.set_fw_table(cg.LpmTable(fw_rules, 1024, 24))
        ctx.set_route_lpm(rt)
        dp, dr = ctx.alloc(pk.nbytes), ctx.alloc(n * 8)
        dp.upload(pk)
        batches = [cg.make_batch(dp, B, dr, pkts_offset=i * B * 64, results_offset=i * B * 8) for i in range(nb)]
        med, lo, hi = timed(ctx, lambda: ctx.submit(batches), a.reps, a.warmup)
        ctx.sync()
        res = dr.download(cg.RESULT_DT, 1 << 16)
        want = rt.lookup_words(dst[:1 << 16])
        assert np.array_equal(res["route_nh"], want & 0xFFFFFF)
        print(json.dumps({"case": "pipeline F|L one-shot, 64-byte frames, routes100k dir-plain + fw1k lds",
                          "route_form": ctx.route_form(), "n": n, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                          "max_ms": round(hi, 4), "mpkt_s": round(n / med / 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--skip-1m", action="store_true")
    a = ap.parse_args()
    fw = cg.gen_rules(0x5EED1002, 1000, cg.GEN_FW, 20)
    r100k = cg.gen_rules(0x5EED2003, 100000, cg.GEN_ROUTES, 0)
    case("fw1k", F, cg.LpmTable(fw, 1024, 24), fw, 0, "plain", "lds", a)
    t100k = cg.LpmTable(r100k, 1 << 20, 1 << 16, False)
    for name, flags, tbl8, form in (("routes100k", DIR, "plain", "dir"), ("routes100k", DIR, "packed", None),
                                    ("routes100k", cg.CFG_LPM_TRIE, "plain", "trie"),
                                    ("routes100k", cg.CFG_LPM_BKT, "plain", "bkt")):
        case(name, L, t100k, r100k, flags, tbl8, form, a)
    if a.pipeline:
        pipeline(fw, r100k, t100k, a)
    if not a.skip_1m:
        r1m = cg.gen_rules(0x5EED2005, 1000000, cg.GEN_ROUTES, 0)
        t1m = cg.LpmTable(r1m, 1 << 21, 1 << 18, False)
        held = t1m.rules()
        # $COP_TBL8=auto: the library's default (packed groups once they pass 16 MiB)
        for flags, form in ((DIR, None), (cg.CFG_LPM_BKT, "bkt")):
            case("routes1m", L, t1m, held, flags, "auto", form, a)


if __name__ == "__main__":
    main()
