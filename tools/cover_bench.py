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
--diff: the table diff (cls_table_diff) instead -- each table against its
edit (one live rule's action flipped, one live rule deleted), three ways in one
process, alternated, each the best of --rounds windows of --iters back-to-back
calls:
B: cls_table_diff with device outputs (everything but the records' download);
A: two cls_classify_rules(CLS_F_DEVICE) calls, one per table, over the joint
   cells prebuilt in HBM, which leaves 2 x 5 B per cell (verdict and rule) to
   download and compare on the host -- that is not in A's time;
C: two cls_table_cover calls with device outputs, one per table.
--kernel-stats then traces the B calls (tdiff_count, tdiff_emit,
reach_diff_scan and cover's kernels).
--need: the rule necessity sweep (cls_table_need) instead, in one process,
alternated, each the best of --rounds windows of --iters back-to-back calls:
B: cls_table_need with every device output, and B_no_free without free_out
   (no second pass over the cells);
A: cls_table_cover with device outputs on the same table -- the floor of one
   pass over the cells;
C: what a user does without the call, per rule: put the list without r and
   cls_table_diff against it; timed for 16 rules and EXTRAPOLATED to R.
Once each: cls_table_need_host, the counts per need value, the rounds and the
result size of the minimizing round loop (checked with cls_table_diff), and the
same sweep with need_cols_lds=0.  --kernel-stats then traces the B calls
(need_bits, need_cells, need_mark, need_free, need_finish and cover's folds).
usage: python tools/cover_bench.py --af 4|16 [--diff | --need] [--kernel-stats]
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


def edited(eng, rules, af):
    """rules with the action of the live rule of most cells flipped (DENY <-> PERMIT; REFLECT -> DENY) and the next
    live rule deleted."""
    import copy
    from vpp_amd import model as M
    tb = eng.put_table("edit", rules)
    cov = eng.table_cover(tb, af=af)
    eng.del_table(tb)
    ks = [k for k in range(len(rules)) if cov["live"][k] and rules[k].actions is not None]
    ks.sort(key=lambda k: (-int(cov["cells"][k]), k))
    out = [copy.deepcopy(r) for r in rules]
    out[ks[0]].actions.acl_action = M.PERMIT if out[ks[0]].actions.acl_action == M.DENY else M.DENY
    del out[ks[1]]
    return out, ks[:2]


def measure_diff(a):
    import torch
    from vpp_amd.engine import Engine
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    sync = torch.cuda.synchronize
    i64, i32 = torch.int64, torch.int32
    out = []
    for name, rules in tables():
        other, picked = edited(eng, rules, a.af)
        ta, tb = eng.put_table(name, rules), eng.put_table(name + " edited", other)
        ra, rb = len(rules) + 1, len(other) + 1
        cap = eng.table_diff(ta, tb, af=a.af, rec_cap=0)["n_rec"] + 16
        host = eng.table_diff(ta, tb, af=a.af, rec_cap=cap)
        shapes = ((1,), (4, 4), (1, 4), (ra,), (ra, 4), (rb,), (rb, 4), (cap, 8), (1,))
        res = [torch.empty(sh, dtype=dt, device="cuda") for sh, dt in zip(shapes, (i64, i64, i32, i64, i32, i64, i32, i32, i64))]
        line = {"table": name, "rules": len(rules), "flipped_deleted": picked, "joint_dims_Ks_Kd_Kt_Ku": host["dims"],
                "cells": host["n_cells"], "n_diff": host["n_diff"], "n_rec": host["n_rec"],
                "pairs": host["pairs"].tolist()}
        run_b = lambda: eng.table_diff(ta, tb, af=a.af, rec_cap=cap, out=res)
        if a.child:
            piped(run_b, a.iters, sync)
            out.append(line)
            continue
        cov = [(torch.empty(r, dtype=torch.uint8, device="cuda"), torch.empty((r, 4), dtype=i32, device="cuda"),
                torch.empty(r, dtype=i64, device="cuda"), torch.empty(1, dtype=i32, device="cuda")) for r in (ra, rb)]

        def run_c():
            eng.table_cover(ta, af=a.af, out=cov[0])
            eng.table_cover(tb, af=a.af, out=cov[1])
        c, _ = cells(list(rules) + list(other), a.af)
        d = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v.view(np.int16) if v.dtype == np.uint16
                                 else v).to("cuda") for k, v in c.items()}
        n = len(c["proto"])
        va, vb = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2))
        ha, hb = (torch.empty(n, dtype=i32, device="cuda") for _ in range(2))

        def run_a():
            eng.classify_rules(ta, d["src"], d["dst"], d["dport"], d["proto"], va, ha)
            eng.classify_rules(tb, d["src"], d["dst"], d["dport"], d["proto"], vb, hb)
        best = {"B": 1e9, "A": 1e9, "C": 1e9}
        for _ in range(a.rounds):                       # alternated
            for key, fn in (("B", run_b), ("A", run_a), ("C", run_c)):
                best[key] = min(best[key], piped(fn, a.iters, sync))
        line.update({k + "_ms": round(v, 4) for k, v in best.items()})
        line["A_left_to_download_MB"] = round(2 * 5 * n / 1e6, 1)
        t0 = time.perf_counter()
        eng.table_diff(ta, tb, af=a.af, rec_cap=cap)
        line["B_host_form_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
        sync()
        line["A_equals_B"] = bool(int((va != vb).sum().item()) == host["n_diff"] and n == host["n_cells"])
        dev = run_b()
        sync()
        line["B_device_equals_host"] = bool(
            int(dev["n_diff"].item()) == host["n_diff"] and int(dev["n_rec"].item()) == host["n_rec"] and
            dev["records"].cpu().numpy()[:host["n_rec"]].tobytes() == host["records"].tobytes() and
            dev["wit_a"].cpu().numpy().tobytes() == host["wit_a"].tobytes() and
            dev["wit_b"].cpu().numpy().tobytes() == host["wit_b"].tobytes())
        line["B_over_C"], line["B_over_A"] = round(best["B"] / best["C"], 3), round(best["B"] / best["A"], 3)
        out.append(line)
        eng.del_table(ta)
        eng.del_table(tb)
        del d, va, vb, ha, hb
    eng.close()
    return out


def measure_need(a):
    import torch
    from vpp_amd.engine import Engine, minimize_rounds
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    sync = torch.cuda.synchronize
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    out = []
    for name, rules in tables():
        tb = eng.put_table(name, rules)
        r = len(rules)
        res = [torch.empty(r, dtype=u8, device="cuda"), torch.empty(r, dtype=u8, device="cuda"),
               torch.empty(r + 1, dtype=i64, device="cuda"), torch.empty(r, dtype=i64, device="cuda"),
               torch.empty((r, 4), dtype=i32, device="cuda"), torch.empty(4, dtype=i32, device="cuda")]
        run_b = lambda: eng.table_need(tb, out=res)
        run_b1 = lambda: eng.table_need(tb, out=[res[0], False] + res[2:])
        if a.child:
            piped(run_b, a.iters, sync)
            out.append({"table": name})
            eng.del_table(tb)
            continue
        host = eng.table_need(tb)
        line = {"table": name, "rules": r, "dims_Ks_Kd_Kt_Ku": host["dims"], "cells": host["n_cells"],
                "W_words": max(1, (r + 63) // 64), "counts_skipped_dead_redundant_needed": host["counts"].tolist(),
                "free": int(host["free"].sum()), "default_reachable": bool(host["first"][r])}
        cov = (torch.empty(r + 1, dtype=u8, device="cuda"), torch.empty((r + 1, 4), dtype=i32, device="cuda"),
               torch.empty(r + 1, dtype=i64, device="cuda"), torch.empty(1, dtype=i32, device="cuda"))
        run_a = lambda: eng.table_cover(tb, af=a.af, out=cov)
        best = {"B": 1e9, "B_no_free": 1e9, "A": 1e9}
        for _ in range(a.rounds):                       # alternated
            for key, fn in (("B", run_b), ("B_no_free", run_b1), ("A", run_a)):
                best[key] = min(best[key], piped(fn, a.iters, sync))
        line.update({k + "_ms": round(v, 4) for k, v in best.items()})
        line["B_over_A"] = round(best["B"] / best["A"], 3)
        eng.set_option("need_cols_lds", 0)
        line["B_cols_global_ms"] = round(min(piped(run_b, a.iters, sync) for _ in range(a.rounds)), 4)
        glob_form = eng.table_need(tb)
        eng.set_option("need_cols_lds", None)
        line["cols_global_equals_lds"] = all(glob_form[k].tobytes() == host[k].tobytes() for k in
                                             ("need", "free", "first", "changed", "witness", "counts"))
        t0 = time.perf_counter()
        eng.table_need(tb)
        line["B_host_form_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
        dev = run_b()
        sync()
        line["B_device_equals_host"] = all(dev[k].cpu().numpy().tobytes() == host[k].tobytes() for k in
                                           ("need", "free", "first", "changed", "witness", "counts"))
        cvr = eng.table_cover(tb, af=a.af)
        line["first_equals_cover_cells"] = bool(np.array_equal(host["first"], cvr["cells"]))
        # C: put + diff per rule, 16 rules spread over the list
        picks = sorted(set(int(x) for x in np.linspace(0, r - 1, 16)))
        t0 = time.perf_counter()
        agree = True
        for k in picks:
            t2 = eng.put_table(name + " without", rules[:k] + rules[k + 1:])
            d = eng.table_diff(tb, t2, af=a.af, rec_cap=0)
            eng.del_table(t2)
            agree = agree and d["equal"] == (host["need"][k] != 3)
        per = (time.perf_counter() - t0) / len(picks) * 1e3
        line["C_put_and_diff_ms_per_rule"] = round(per, 3)
        line["C_extrapolated_to_R_ms"] = round(per * r, 1)
        line["C_agrees_with_need_on_the_16"] = bool(agree)
        t0 = time.perf_counter()
        cpu = Engine.table_need_host(rules)
        line["need_host_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        line["need_host_equals_device"] = all(cpu[k].tobytes() == host[k].tobytes() for k in
                                              ("need", "free", "first", "changed", "witness", "counts"))
        t0 = time.perf_counter()
        kept, rounds = minimize_rounds(lambda skip: eng.table_need(tb, skip=skip), r)
        line["minimize_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        line["minimize_rounds"], line["minimized_rules"] = len(rounds), len(kept)
        line["removed_per_round"] = [len(x) for x in rounds]
        t2 = eng.put_table(name + " minimized", [rules[k] for k in kept])
        line["minimized_diffs_equal"] = bool(eng.table_diff(tb, t2, af=a.af, rec_cap=0)["equal"])
        eng.del_table(t2)
        out.append(line)
        eng.del_table(tb)
    eng.close()
    return out


def kernel_stats(a):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--af", str(a.af), "--iters", str(a.iters),
               "--rounds", "1", "--tiles", str(a.stats_tile)] + [x for o in a.opt for x in ("--opt", o)] + \
              (["--diff"] if a.diff else []) + (["--need"] if a.need else [])
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
                        "classify4_linear", "tdiff_count", "tdiff_emit", "reach_diff_scan", "need_bits", "need_cells",
                        "need_mark", "need_free", "need_finish"):
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
        return {"cover_tile": "default" if a.diff or a.need else a.stats_tile, "both_tables_together": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--af", type=int, default=4, choices=[4, 16])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="the best of this many timed windows")
    ap.add_argument("--tiles", type=int, nargs="+", default=[1 << 20, 1 << 22, 1 << 24])
    ap.add_argument("--chunk", type=int, default=1 << 28, help="A: cells per prebuilt chunk")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--diff", action="store_true", help="the table diff (cls_table_diff) against two classify calls "
                                                        "and two cover sweeps")
    ap.add_argument("--need", action="store_true", help="the rule necessity sweep (cls_table_need) against one cover "
                                                        "sweep and against put + diff per rule")
    ap.add_argument("--stats-tile", type=int, default=1 << 22)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE")
    a = ap.parse_args()
    from vpp_amd import _abi
    lines = measure_need(a) if a.need else measure_diff(a) if a.diff else measure(a)
    if a.child:
        return
    res = {"bench": "table_need" if a.need else "table_diff" if a.diff else "cover", "af": a.af, "iters": a.iters, "rounds": a.rounds, "tables": lines,
           "sources": _abi.source_hash()}
    if a.kernel_stats:
        res["kernel_stats"] = kernel_stats(a)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
