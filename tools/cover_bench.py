#!/usr/bin/env python3
"""A / B of the rule coverage sweep (cls_table_cover), one JSON line.

Tables: the config-3 global table (vpp_amd.workload) and the pod's ingress
list of the 20-block gen-policy workload (tools/genpolicy_bench.py's), in the
layout given by --af.
B: cls_table_cover with device outputs -- cells expanded, classified and
   folded on the device; per call, `iters` calls queued back to back with one
   wait at the end, and once as the host form (outputs downloaded).
A: cls_classify_rules(CLS_F_DEVICE) over the same cells prebuilt in HBM (the
   arrays cover_cases-style numpy builds from cls_cover_classes and
   cls_port_classes, in as many chunks as --chunk allows), which leaves 4 B
   per cell to download and fold on the host; that download and a numpy fold
   (bincount and first index per rule) are timed once and reported beside A,
   not inside it.
B / A is reported per table, B also at every --tiles value (cover_tile).
--kernel-stats: the B calls once more in a child under rocprofv3
--kernel-trace --stats (a run of its own), average microseconds per launch of
cover_expand4 / 16, cover_fold, cover_finish and of every other kernel the
sweep launched (the classify kernels in slot mode and slot_rules_kernel).
usage: python tools/cover_bench.py --af 4|16 [--kernel-stats]
"""
import argparse
import csv
import glob
import json
import os
import random
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tables():
    from vpp_amd import configurator as C
    from vpp_amd import workload
    from vpp_amd.renderer.api import PodID
    from vpp_amd.renderer.traffic import compile_rules
    acl, _, _ = workload.config(3)
    pol = C.gen_policy(random.Random(20), num_cidrs=20)
    txn = C.PolicyConfigurator({PodID("db", "default"): "10.1.1.1"}).new_txn(False)
    return [("config3", acl.rules), ("genpolicy20_ingress", compile_rules(txn.generate_rules(C.MATCH_INGRESS, [pol])))]


def cells(rules, af):
    """The sweep's cells as host arrays, cell = (s Kd + d) T + j."""
    from vpp_amd import _abi
    from vpp_amd.engine import Engine
    cr = _abi.CRules(rules)
    slo, dlo = Engine.cover_classes(cr, 0), Engine.cover_classes(cr, 1)
    t, u = Engine.port_classes(cr, 0), Engine.port_classes(cr, 1)
    proto = np.concatenate([np.zeros(len(t)), np.ones(len(u)), [2, 3]]).astype(np.uint8)
    dport = np.concatenate([t, u, [0, 0]]).astype(np.uint16)
    ks, kd, T = len(slo), len(dlo), len(proto)
    src, dst = np.repeat(slo, kd * T), np.tile(np.repeat(dlo, T), ks)
    if af == 16:
        def wide(a):
            out = np.zeros((len(a), 16), np.uint8)
            out[:, 10:12] = 0xFF
            out[:, 12:] = a.astype(">u4").view(np.uint8).reshape(-1, 4)
            return out
        src, dst = wide(src), wide(dst)
    return dict(src=src, dst=dst, dport=np.tile(dport, ks * kd), proto=np.tile(proto, ks * kd)), (ks, kd, len(t), len(u))


def piped(fn, iters, sync):
    """ms per call of `iters` calls queued back to back, one wait at the end (after a warm call)."""
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters * 1e3


def measure(a):
    import torch
    from vpp_amd.engine import Engine
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    sync = torch.cuda.synchronize
    out = []
    for name, rules in tables():
        tb = eng.put_table(name, rules)
        r = len(rules) + 1
        res = (torch.empty(r, dtype=torch.uint8, device="cuda"), torch.empty((r, 4), dtype=torch.int32, device="cuda"),
               torch.empty(r, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
        host = eng.table_cover(tb, af=a.af)
        line = {"table": name, "rules": len(rules), "dims_Ks_Kd_Kt_Ku": host["dims"], "cells": host["n_cells"],
                "dead": host["n_dead"], "default_reachable": bool(host["live"][-1])}
        by_tile = {}
        for tile in a.tiles:
            eng.set_option("cover_tile", tile)
            by_tile[str(tile)] = round(min(piped(lambda: eng.table_cover(tb, af=a.af, out=res), a.iters, sync)
                                           for _ in range(a.rounds)), 4)
        eng.set_option("cover_tile", None)
        line["B_ms_by_cover_tile"] = by_tile
        if a.child:
            out.append(line)
            eng.del_table(tb)
            continue
        line["B_ms"] = round(min(piped(lambda: eng.table_cover(tb, af=a.af, out=res), a.iters, sync)
                                 for _ in range(a.rounds)), 4)
        t0 = time.perf_counter()
        eng.table_cover(tb, af=a.af)
        line["B_host_form_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
        dev = eng.table_cover(tb, af=a.af, out=res)
        sync()
        line["B_device_equals_host"] = bool(np.array_equal(dev["live"].cpu().numpy(), host["live"]) and
                                            dev["witness"].cpu().numpy().tobytes() == host["witness"].tobytes() and
                                            np.array_equal(dev["cells"].cpu().numpy().view(np.uint64), host["cells"]))
        # A: the same cells prebuilt in HBM, in chunks
        c, _ = cells(rules, a.af)
        n = len(c["proto"])
        chunks = []
        for off in range(0, n, a.chunk):
            d = {k: torch.from_numpy(v[off:off + a.chunk].view(np.int32) if v.dtype == np.uint32 else
                                     v[off:off + a.chunk].view(np.int16) if v.dtype == np.uint16 else
                                     v[off:off + a.chunk]).to("cuda") for k, v in c.items()}
            d["rules"] = torch.empty(len(d["proto"]), dtype=torch.int32, device="cuda")
            chunks.append(d)

        def run_a():
            for d in chunks:
                eng.classify_rules(tb, d["src"], d["dst"], d["dport"], d["proto"], None, d["rules"])
        line["A_chunks"] = len(chunks)
        line["A_array_MB"] = round(sum(v.nbytes for v in c.values()) / 1e6, 1)
        line["A_ms"] = round(min(piped(run_a, a.iters, sync) for _ in range(a.rounds)), 4)
        t0 = time.perf_counter()
        hit = np.concatenate([d["rules"].cpu().numpy() for d in chunks]).astype(np.int64)
        t1 = time.perf_counter()
        count = np.bincount(hit, minlength=r)
        k, first = np.unique(hit, return_index=True)
        t2 = time.perf_counter()
        line["A_download_ms"], line["A_host_fold_ms"] = round((t1 - t0) * 1e3, 3), round((t2 - t1) * 1e3, 3)
        line["A_equals_B"] = bool(np.array_equal(count.astype(np.uint64), host["cells"]) and
                                  np.array_equal(k, np.flatnonzero(host["live"])))
        line["B_over_A"] = round(line["B_ms"] / line["A_ms"], 3)
        out.append(line)
        eng.del_table(tb)
    eng.close()
    return out


def kernel_stats(a):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--af", str(a.af), "--iters", str(a.iters),
               "--rounds", "1", "--tiles", str(a.stats_tile)] + [x for o in a.opt for x in ("--opt", o)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": r.stderr[-400:]}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv"}
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row["Name"]
            for key in ("cover_expand4", "cover_expand16", "cover_fold_bins", "cover_fold", "cover_finish", "slot_rules_kernel",
                        "classify4_linear"):
                if key in name:
                    name = key
                    break
            else:
                name = name.replace("(anonymous namespace)::", "").replace("cls::", "").replace("void ", "")[:48]
            e = out.setdefault(name, {"calls": 0, "total_ns": 0})
            e["calls"] += int(row["Calls"])
            e["total_ns"] += int(row["TotalDurationNs"])
        for e in out.values():
            e["avg_us"] = round(e["total_ns"] / max(1, e["calls"]) / 1e3, 2)
        return {"cover_tile": a.stats_tile, "both_tables_together": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--af", type=int, default=4, choices=[4, 16])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="the best of this many timed windows")
    ap.add_argument("--tiles", type=int, nargs="+", default=[1 << 20, 1 << 22, 1 << 24])
    ap.add_argument("--chunk", type=int, default=1 << 28, help="A: cells per prebuilt chunk")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--stats-tile", type=int, default=1 << 22)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE")
    a = ap.parse_args()
    from vpp_amd import _abi
    lines = measure(a)
    if a.child:
        return
    res = {"bench": "cover", "af": a.af, "iters": a.iters, "rounds": a.rounds, "tables": lines,
           "sources": _abi.source_hash()}
    if a.kernel_stats:
        res["kernel_stats"] = kernel_stats(a)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
