#!/usr/bin/env python3
"""Time live rule updates against the whole-table upload they replace.

On the 100k-route table, on one COP_CFG_LIVE_TABLES context, three changes:
one /24 added, 1,000 mixed changes (adds, next-hop overwrites, deletes) and
one /8 added. Each is timed as the host wall clock from the call of
cop_update_route_lpm to the return of cop_sync, and compared with
cop_set_route_lpm of the same resulting table followed by cop_sync (the path
that existed before, on the same context). The change is undone, untimed,
between repetitions; the first repetitions warm up. Prints one JSON line per
case (medians, min, max in ms, the ratio, the update's report).

    python tools/table_update.py [--reps 15] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ghost-dataplane_amd"))
import copgpu as cg  # noqa: E402


def mixed_changes(rules, rng, n=1000):
    """(apply, undo) op lists: 400 fresh host routes and /24s, 300 next-hop
    overwrites, 300 deletes, over distinct rules."""
    pick = rng.choice(len(rules), 600, replace=False)
    apply, undo = [], []
    held = {(int(r["ip"]), int(r["depth"])) for r in rules}
    while len(apply) < 400 * n // 1000:
        depth = int(rng.choice([24, 32]))
        ip = int(rng.integers(0, 1 << 32)) & (0xFFFFFFFF << (32 - depth)) & 0xFFFFFFFF
        if (ip, depth) in held:
            continue
        held.add((ip, depth))
        apply.append(("add", ip, depth, int(rng.integers(1, 1 << 24))))
        undo.append(("del", ip, depth))
    for k in pick[:300]:
        r = rules[k]
        apply.append(("add", int(r["ip"]), int(r["depth"]), int(r["next_hop"]) ^ 1))
        undo.append(("add", int(r["ip"]), int(r["depth"]), int(r["next_hop"])))
    for k in pick[300:]:
        r = rules[k]
        apply.append(("del", int(r["ip"]), int(r["depth"])))
        undo.append(("add", int(r["ip"]), int(r["depth"]), int(r["next_hop"])))
    return apply, undo


def run_ops(t, ops):
    for op in ops:
        rc = t.add(*op[1:]) if op[0] == "add" else t.delete(*op[1:])
        if rc != 0:
            raise RuntimeError(f"{op}: {rc}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--routes", type=int, default=100000)
    a = ap.parse_args()
    if cg.device_count() < 1:
        sys.exit("table_update: no GPU visible")
    rules = cg.gen_rules(0x5EED2003, a.routes, cg.GEN_ROUTES, 0)
    t = cg.LpmTable(rules, 1 << 20, 1 << 16, False)
    held = t.rules()
    rng = np.random.default_rng(0x7AB1E)
    free24 = next(ip for ip in (0xC6336400, 0xCB007100, 0xC0000200)
                  if t.is_rule_present(ip, 24)[0] == 0)
    free8 = next(ip for ip in range(0x0A000000, 0xE0000000, 0x01000000) if t.is_rule_present(ip, 8)[0] == 0)
    cases = {
        "one_slash24": ([("add", free24, 24, 77)], [("del", free24, 24)]),
        "mixed_1000": mixed_changes(held, rng),
        "one_slash8": ([("add", free8, 8, 78)], [("del", free8, 8)]),
    }
    with cg.Context(stages=cg.STAGE_FW | cg.STAGE_LPM, flags=cg.CFG_LIVE_TABLES) as ctx:
        ctx.set_route_lpm(t)
        ctx.sync()
        for name, (apply, undo) in cases.items():
            upd, full, rep = [], [], None
            for i in range(a.warmup + a.reps):
                run_ops(t, apply)
                t0 = time.perf_counter()
                rep = ctx.update_route_lpm(t)
                ctx.sync()
                t1 = time.perf_counter()
                ctx.set_route_lpm(t)
                ctx.sync()
                t2 = time.perf_counter()
                assert rep["full"] == 0, rep
                run_ops(t, undo)
                ctx.update_route_lpm(t)
                ctx.sync()
                if i >= a.warmup:
                    upd.append((t1 - t0) * 1e3)
                    full.append((t2 - t1) * 1e3)
            mu, mf = statistics.median(upd), statistics.median(full)
            print(json.dumps({"case": name, "routes": a.routes, "reps": a.reps,
                              "update_ms": {"median": round(mu, 4), "min": round(min(upd), 4), "max": round(max(upd), 4)},
                              "set_route_lpm_ms": {"median": round(mf, 3), "min": round(min(full), 3),
                                                   "max": round(max(full), 3)},
                              "ratio_full_over_update": round(mf / mu, 1), "report": rep}), flush=True)


if __name__ == "__main__":
    main()
