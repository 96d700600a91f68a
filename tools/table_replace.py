#!/usr/bin/env python3
"""Time whole-table replacement against the whole-table upload.

On one COP_CFG_LIVE_TABLES context per table, two table objects A and B of
the same size take turns, first through cop_replace_*, then through
cop_set_* (the path that existed before, on the same context). A repetition
is the host wall clock from the call to the return of cop_sync; the first
repetitions of each loop warm up. Tables:
the 100k-route table, the 1k firewall table, and with --million the 1M-route
table of the benchmark's fw_lpm_1m workload. Prints one JSON line per table
(medians, min, max in ms, the ratio, the replacement's report).

    python tools/table_replace.py [--reps 15] [--warmup 3] [--million]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ghost-dataplane_amd"))
import copgpu as cg  # noqa: E402


def tables(name):
    """(is_fw, table A, table B, context flags)"""
    if name == "routes_100k":
        mk = lambda seed: cg.LpmTable(cg.gen_rules(seed, 100000, cg.GEN_ROUTES, 0), 1 << 20, 1 << 16, False)  # noqa: E731
        return False, mk(0x5EED2003), mk(0x5EED2004), 0
    if name == "fw_1k":
        mk = lambda seed: cg.LpmTable(cg.gen_rules(seed, 1000, cg.GEN_FW, 20), 1024, 24, True)  # noqa: E731
        return True, mk(0x5EED1002), mk(0x5EED1003), 0
    if name == "routes_1m":
        mk = lambda seed: cg.LpmTable(cg.gen_rules(seed, 1000000, cg.GEN_ROUTES, 0), 1000000, 1 << 20, False)  # noqa: E731
        return False, mk(0x5EED2005), mk(0x5EED2006), 0
    raise ValueError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--million", action="store_true", help="also the 1M-route table")
    ap.add_argument("--only", default=None, help="one table: routes_100k, fw_1k or routes_1m")
    a = ap.parse_args()
    if cg.device_count() < 1:
        sys.exit("table_replace: no GPU visible")
    names = [a.only] if a.only else ["routes_100k", "fw_1k"] + (["routes_1m"] if a.million else [])
    for name in names:
        is_fw, ta, tb, flags = tables(name)
        with cg.Context(stages=cg.STAGE_FW | cg.STAGE_LPM, flags=cg.CFG_LIVE_TABLES | flags) as ctx:
            replace = ctx.replace_fw_table if is_fw else ctx.replace_route_lpm
            upload = ctx.set_fw_table if is_fw else ctx.set_route_lpm
            upload(ta)
            ctx.sync()
            # The two paths are timed in loops of their own: cop_set_* frees and
            # reallocates the image at the size of its table, so a replacement
            # right behind it may have to allocate a larger tbl8 again, which a
            # context that is only ever replaced pays once. That first
            # replacement is timed on its own ("first_replace_ms").
            rep_ms, set_ms, rep = [], [], None
            t0 = time.perf_counter()
            replace(tb)
            ctx.sync()
            first_ms = (time.perf_counter() - t0) * 1e3
            for i in range(a.warmup + a.reps):
                t = ta if i % 2 == 0 else tb
                t0 = time.perf_counter()
                rep = replace(t)
                ctx.sync()
                t1 = time.perf_counter()
                assert rep["full"] == 0, rep
                if i >= a.warmup:
                    rep_ms.append((t1 - t0) * 1e3)
            audit = ctx.lookup_audit(cg.STAGE_FW if is_fw else cg.STAGE_LPM, t)[0]
            assert audit["n_mismatch"] == 0 and audit["stale"] == 0, audit
            for i in range(a.warmup + a.reps):
                t = ta if i % 2 == 0 else tb
                t0 = time.perf_counter()
                upload(t)
                ctx.sync()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    set_ms.append((t1 - t0) * 1e3)
            mr, ms = statistics.median(rep_ms), statistics.median(set_ms)
            print(json.dumps({"table": name, "reps": a.reps, "form": ctx.lookup_form(cg.STAGE_FW if is_fw else cg.STAGE_LPM),
                              "replace_ms": {"median": round(mr, 4), "min": round(min(rep_ms), 4),
                                             "max": round(max(rep_ms), 4)},
                              "first_replace_ms": round(first_ms, 3),
                              "set_ms": {"median": round(ms, 3), "min": round(min(set_ms), 3), "max": round(max(set_ms), 3)},
                              "ratio_set_over_replace": round(ms / mr, 1), "report": rep}), flush=True)


if __name__ == "__main__":
    main()
