#!/usr/bin/env python3
"""The reachability matrix (cls_reach_matrix) against the device-batch path it
is built on.

Layout: conn_bench.py's ACL set -- the config-3 global ACL (IPv4; --af 16: the
config-5 table) on if0/if1 (in) and if0/if2 (out), --locals random local ACLs
on 77 further interfaces -- and N endpoints (half on the global ACL's
interfaces with pod addresses, half on any interface with addresses around
the locals' prefixes) x 4 probes (TCP and UDP on table ports, TCP 80,
protocol 47).  For every N of --endpoints and every --tiles value it times

  t_reach    cls_reach_matrix with device outputs (verdicts, histogram, allow
             counts), --iters calls back to back, one wait at the end;
  t_connect  cls_connect_batch(CLS_F_DEVICE) over the same P N^2 connections
             prebuilt in HBM (in batches of the tile size), the same way;

and prints one JSON line per N: t_reach / t_connect per tile, the connection
stream floor of the prebuilt rows (cls_stream_floor_conn, IPv4), and the
parity of the whole matrix with the prebuilt batch and of a >= 20k-cell sample
with orc_test_connection_hits.  --kernel-stats runs the same measurement once
more in a child of its own under rocprofv3 --kernel-trace --stats, at the one
tile size --stats-tile, and adds the average time per launch of reach_expand4
/ reach_expand16, reach_reduce and connect_kernel.

usage: python tools/reach_bench.py [--af 4|16] [--locals 12] [--endpoints 1024,2048]
           [--tiles 1048576,4194304,16777216] [--iters 9] [--kernel-stats]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

N_PROBES = 4


def setup(eng, af, n_local, n):
    """ACLs on the engine; (bind, by_name, ifs, endpoint interface index,
    addresses, probes)."""
    from aclgen import random_traffic, random_traffic16
    from test_gpu_connect_scale import build
    rng = np.random.default_rng(11)
    half = rng.random(n) < 0.5
    if af == 16:
        import oracle
        from conn_bench import build16
        ifs, bind, by_name, pool, spec = build16(eng, 0, n_local)
        addrs = random_traffic16(7, n, pool)["src"]
        addrs[half] = oracle.gen_traffic_v16(spec, 0, n)["src"][half]
        tport = int(spec["ports"][0])
    else:
        ifs, bind, by_name, pool, spec = build(eng, 0, cfg=3, n_local=n_local)
        addrs = random_traffic(7, n, pool)["src"]
        addrs[half] = rng.choice(spec["pod_ips"].astype(np.uint32), half.sum())
        tport = int(spec["ports"][0])
    at = np.where(half, rng.integers(0, 2, n), rng.integers(0, len(ifs), n))
    probes = (np.array([0, 1, 0, 47], np.uint8), np.array([40000, 53000, 41000, 0], np.uint16),
              np.array([tport, 53, 80, 0], np.uint16))
    return bind, by_name, ifs, at, addrs, probes


def expand(at, addrs, pr, sp, dp):
    n, p = len(at), len(pr)
    pi = np.repeat(np.arange(p), n * n)
    si = np.tile(np.repeat(np.arange(n), n), p)
    di = np.tile(np.arange(n), n * p)
    return si, di, pi, {"src": addrs[si], "dst": addrs[di], "proto": pr[pi], "sport": sp[pi], "dport": dp[pi]}


def piped(fn, iters, sync):
    """ms per call of `iters` calls queued back to back, one wait at the end
    (after a warm call: plans, uploads, scratch)."""
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters * 1e3


def measure(a, n):
    import torch
    from test_gpu_connect_scale import oracle_connections
    from vpp_amd import _abi
    from vpp_amd.engine import Engine, _ptr
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    bind, by_name, ifs, at, addrs, (pr, sp, dp) = setup(eng, a.af, a.locals, n)
    ids = np.array([eng.if_id(x) for x in ifs], np.uint32)
    cells = N_PROBES * n * n
    L, sync = _abi.lib(), torch.cuda.synchronize
    # the matrix call, its arguments built once
    ep_if = np.ascontiguousarray(ids[at], np.uint32)
    ep_addr = np.ascontiguousarray(addrs, np.uint8 if a.af == 16 else np.uint32)
    spec = _abi.ReachSpec(a.af, n, _ptr(ep_if), None if a.af == 16 else _ptr(ep_addr),
                          _ptr(ep_addr) if a.af == 16 else None, N_PROBES, _ptr(pr), _ptr(sp), _ptr(dp))
    dv = torch.empty(cells, dtype=torch.uint8, device="cuda")
    dh = torch.empty((N_PROBES, 4), dtype=torch.int64, device="cuda")
    da = torch.empty((N_PROBES, n), dtype=torch.int32, device="cuda")

    def reach(verdicts=True):
        rc = L.cls_reach_matrix(eng.h, C.byref(spec), _ptr(dv) if verdicts else None, _ptr(dh), _ptr(da),
                                _abi.F_DEVICE | (0 if verdicts else _abi.F_NO_VERDICT), None)
        assert rc == 0, L.cls_last_error(eng.h)
    # the same connections prebuilt in HBM
    si, di, pi, tr = expand(at, addrs, pr, sp, dp)
    host = (ids[at[si]], ids[at[di]], tr["src"], tr["dst"], tr["proto"], tr["sport"], tr["dport"])
    dargs = [torch.from_numpy(np.ascontiguousarray(x).view({4: np.int32, 2: np.int16, 1: np.uint8}[x.dtype.itemsize]))
             .to("cuda") for x in host]
    cv = torch.empty(cells, dtype=torch.uint8, device="cuda")

    def connect_call(first, cnt):
        sl = [x[first:first + cnt] for x in dargs]
        if a.af == 16:
            pk = _abi.PktSoa(_abi.AF_V16, None, None, _ptr(sl[2]), _ptr(sl[3]), _ptr(sl[5]), _ptr(sl[6]), _ptr(sl[4]))
        else:
            pk = _abi.PktSoa(_abi.AF_V4, _ptr(sl[2]), _ptr(sl[3]), None, None, _ptr(sl[5]), _ptr(sl[6]), _ptr(sl[4]))
        cs = _abi.ConnSoa(pk, _ptr(sl[0]), _ptr(sl[1]))
        return cs, cnt, cv.data_ptr() + first, sl

    res = {}
    for tile in a.tiles:
        eng.set_option("reach_tile", tile)
        t_reach = piped(reach, a.iters, sync)
        t_reach_nv = piped(lambda: reach(False), a.iters, sync)
        batches = [connect_call(f, min(tile, cells - f)) for f in range(0, cells, tile)]

        def connect():
            for cs, cnt, out, _ in batches:
                assert L.cls_connect_batch(eng.h, C.byref(cs), cnt, out, _abi.F_DEVICE, None) == 0
        t_conn = piped(connect, a.iters, sync)
        res[str(tile)] = {"t_reach_ms": round(t_reach, 4), "t_connect_ms": round(t_conn, 4),
                          "ratio": round(t_reach / t_conn, 4), "t_reach_no_verdict_ms": round(t_reach_nv, 4),
                          "reach_gconn_s": round(cells / t_reach / 1e6, 2),
                          "connect_gconn_s": round(cells / t_conn / 1e6, 2)}
        reach()
        sync()
        assert torch.equal(dv, cv), "the matrix differs from the prebuilt device batch (tile %d)" % tile
    v = dv.cpu().numpy()
    hist, allow = dh.cpu().numpy(), da.cpu().numpy()
    assert np.array_equal(hist, np.stack([np.bincount(x, minlength=4) for x in v.reshape(N_PROBES, -1)]))
    assert np.array_equal(allow, (v.reshape(N_PROBES, n, n) == 2).sum(axis=2))
    rng = np.random.default_rng(5)
    k = rng.choice(cells, a.cpu_sample, replace=False)
    want, _ = oracle_connections(bind, by_name, ifs, at[si[k]], at[di[k]], {f: x[k] for f, x in tr.items()}, a.af)
    assert np.array_equal(v[k], want), "the matrix differs from the oracle"
    floor = None
    if a.af == 4:
        m = min(cells, 1 << 22)
        floor = eng.stream_floor_conn(*[x[:m] for x in dargs], reps=20) * cells / m
    out = {"metric": "reachability matrix: t_reach / t_connect (cls_reach_matrix with device outputs against "
                     "cls_connect_batch(CLS_F_DEVICE) over the same prebuilt connections)",
           "af": a.af, "endpoints": n, "probes": N_PROBES, "cells": cells, "local_acls": a.locals,
           "global_rules": len(by_name["global"]), "iters": a.iters, "tiles": res,
           "stream_floor_conn_ms": None if floor is None else round(floor, 4),
           "verdicts": np.bincount(v, minlength=4).tolist(),
           "parity": "whole matrix == prebuilt device batch; hist and allow == sums of the cells; %d sampled cells "
                     "bit-exact vs orc_test_connection_hits" % len(k)}
    eng.close()
    return out


def kernel_stats(a, n):
    """The same measurement in a child under rocprofv3 --kernel-trace --stats
    (a run of its own: the timings above are taken without the profiler):
    average ns per call of the matrix's kernels and of connect_kernel."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--af", str(a.af), "--locals", str(a.locals),
               "--endpoints", str(n), "--tiles", str(a.stats_tile), "--iters", str(a.iters),
               "--cpu-sample", "256"] + [x for o in a.opt for x in ("--opt", o)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": r.stderr[-400:]}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv"}
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row["Name"]
            for key in ("reach_expand4", "reach_expand16", "reach_reduce", "connect_kernel"):
                if key in name:
                    e = out.setdefault(key, {"calls": 0, "total_ns": 0})
                    e["calls"] += int(row["Calls"])
                    e["total_ns"] += int(row["TotalDurationNs"])
        for e in out.values():
            e["avg_us"] = round(e["total_ns"] / max(1, e["calls"]) / 1e3, 2)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--af", type=int, default=4, choices=[4, 16])
    ap.add_argument("--locals", type=int, default=12)
    ap.add_argument("--endpoints", default="1024,2048")
    ap.add_argument("--tiles", default="1048576,4194304,16777216")
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--cpu-sample", type=int, default=20000, help="cells checked on the oracle (>= 20000)")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--stats-tile", type=int, default=1 << 22, help="the tile size of the --kernel-stats run")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE")
    a = ap.parse_args()
    a.tiles = [int(x) for x in a.tiles.split(",")]
    for n in [int(x) for x in a.endpoints.split(",")]:
        line = measure(a, n)
        if a.kernel_stats and not a.child:
            from vpp_amd import _abi
            line["kernel_stats"] = dict(kernel_stats(a, n), sources=_abi.source_hash(),
                                        tile=a.stats_tile, note="average per launch at this tile size, under the profiler")
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
