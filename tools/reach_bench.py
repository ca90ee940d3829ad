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

--diff measures the reachability diff (cls_reach_diff) instead: per --locals
value of --diff-locals, N = 2048 endpoints (--endpoints) x 4 probes, in one
process it alternates

  A  cls_reach_matrix(CLS_F_DEVICE) with verdicts, histogram and allow counts;
  B  cls_reach_diff(CLS_F_DEVICE) with the same three outputs plus the changed
     cells' records (cap 1 Mi), their total, the transition counts and the
     changed cells per row, against the matrix of the same ACL set with one
     local ACL deleted and one re-put;

--rounds times --iters calls each, back to back with one wait at the end, and
prints one JSON line per --locals value: the median ms per call of A and B,
B / A and the changed cells (checked against a compare of the two matrices).

--ports measures the port sweep (cls_reach_ports) instead: per --locals value
of --diff-locals it computes the K port classes of the TCP sweep over the
endpoints' ACLs (Engine.port_classes), takes the largest N of 2048, 1024, 512,
256 with K N^2 <= 2^32 rows (a call then stays well under a second) and in one
process alternates

  A  what a caller can do without the call: cls_reach_matrix(CLS_F_DEVICE,
     verdicts to HBM) with P = K probes at the class starts -- K N^2 bytes
     that are still to be downloaded and run-length encoded on the host;
  B  cls_reach_ports(CLS_F_DEVICE) with the ranges (cap: their total), the
     total, the runs and ALLOW ports per pair and the histogram;

and prints one JSON line: the median ms per call of A and B, B / A, K, the
ranges and the bytes each leaves to download (B's runs, ALLOW ports and total
checked against A's verdicts on the device).

--external measures the external sweep (cls_reach_external) instead: per
--locals value of --diff-locals, N = 2048 endpoints x 4 probes x both
directions through the first interface (bound to the global table both ways),
K the address classes of the bound ACLs (Engine.addr_classes); in one process
it alternates

  A  what a caller can do without the call: cls_connect_batch(CLS_F_DEVICE)
     over the same D P N K rows prebuilt in HBM, in batches of B's tiles --
     D P N K verdict bytes that are still to be downloaded and run-length
     encoded on the host;
  B  cls_reach_external(CLS_F_DEVICE) with the ranges (cap: their total), the
     total, the runs and ALLOW addresses per line and the histogram;

and prints one JSON line: the median ms per call of A and B, B / A, K, the
ranges and the bytes each leaves to download (every output of B checked
against the run-length encoding of A's verdicts on the device).

--hops measures the hop closure (cls_reach_hops) instead: per --locals value
of --diff-locals, N = 2048 endpoints (--endpoints) x 4 probes, in one process
it alternates

  A  cls_reach_matrix(CLS_F_DEVICE) with verdicts, histogram and allow counts:
     what a caller can do on the device without the call -- the P N^2 verdicts
     are still to be downloaded and searched on the host;
  B  cls_reach_hops(CLS_F_DEVICE) over the same spec with the hop counts, the
     reach counts and the level histogram;

and prints one JSON line per --locals value: the median ms per call of A and
B, B / A, B at every block height (hops_rows 4, 8, 16), once and labelled as
CPU the host alternative (downloading A's verdicts and running the tests'
numpy search, reach_hops_cases.hops_ref, on them; B's hop counts are checked
against it), and a last line for the matrix form at N = 8192 on a synthetic
random device matrix of out-degree about 2 (checked against a queue search
from 64 sources).

--classes measures the reachability classes (cls_reach_classes) instead: per
--locals value of --diff-locals, N = 2048 endpoints x 4 probes, in one process
it alternates A as above, B = cls_reach_classes(CLS_F_DEVICE) in the
evaluating form with every per-class output (two evaluations), the same with a
device verdict_out (one evaluation, the second pass reads it) and the matrix
form over A's device matrix, and prints one JSON line per --locals value: the
medians, B / A, C, the rounds taken, the bytes each leaves to download and,
once and labelled as CPU, the host alternative (A's verdicts downloaded, then
the tests' numpy grouping, reach_classes_cases.classes_ref; B is checked
against it) and the call over that host matrix.  B returns complete, so its
calls do not overlap; A's are queued back to back.

usage: python tools/reach_bench.py [--af 4|16] [--locals 12] [--endpoints 1024,2048]
           [--tiles 1048576,4194304,16777216] [--iters 9] [--kernel-stats]
       python tools/reach_bench.py --diff [--af 4|16] [--diff-locals 12,64] [--endpoints 2048]
           [--iters 9] [--rounds 7]
       python tools/reach_bench.py --ports [--af 4|16] [--diff-locals 12,64] [--iters 3] [--rounds 5]
           [--kernel-stats]
       python tools/reach_bench.py --external [--af 4|16] [--diff-locals 12,64] [--iters 3] [--rounds 5]
           [--kernel-stats]
       python tools/reach_bench.py --classes [--af 4|16] [--diff-locals 12,64] [--endpoints 2048] [--iters 9]
       python tools/reach_bench.py --hops [--af 4|16] [--diff-locals 12,64] [--endpoints 2048] [--iters 9]
           [--rounds 7] [--kernel-stats]
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


DIFF_CAP = 1 << 20


def measure_diff(a, n, n_local):
    """A / B of cls_reach_matrix and cls_reach_diff on the same engine."""
    import torch
    from aclgen import random_acl, random_acl16
    from vpp_amd import _abi
    from vpp_amd.engine import Engine, _ptr
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    bind, by_name, ifs, at, addrs, (pr, sp, dp) = setup(eng, a.af, n_local, n)
    ids = np.array([eng.if_id(x) for x in ifs], np.uint32)
    cells = N_PROBES * n * n
    L, sync = _abi.lib(), torch.cuda.synchronize
    ep_if = np.ascontiguousarray(ids[at], np.uint32)
    ep_addr = np.ascontiguousarray(addrs, np.uint8 if a.af == 16 else np.uint32)
    spec = _abi.ReachSpec(a.af, n, _ptr(ep_if), None if a.af == 16 else _ptr(ep_addr),
                          _ptr(ep_addr) if a.af == 16 else None, N_PROBES, _ptr(pr), _ptr(sp), _ptr(dp))
    base = torch.empty(cells, dtype=torch.uint8, device="cuda")
    dv = torch.empty(cells, dtype=torch.uint8, device="cuda")
    dh = torch.empty((N_PROBES, 4), dtype=torch.int64, device="cuda")
    da = torch.empty((N_PROBES, n), dtype=torch.int32, device="cuda")
    rec = torch.empty((DIFF_CAP, 4), dtype=torch.int32, device="cuda")
    total = torch.empty(1, dtype=torch.int64, device="cuda")
    trans = torch.empty((N_PROBES, 4, 4), dtype=torch.int64, device="cuda")
    changed = torch.empty((N_PROBES, n), dtype=torch.int32, device="cuda")

    def matrix(v=dv):
        rc = L.cls_reach_matrix(eng.h, C.byref(spec), _ptr(v), _ptr(dh), _ptr(da), _abi.F_DEVICE, None)
        assert rc == 0, L.cls_last_error(eng.h)
    out = _abi.ReachDiffOut(_ptr(dv), _ptr(dh), _ptr(da), _ptr(rec), DIFF_CAP, _ptr(total), _ptr(trans),
                            _ptr(changed))

    def diff():
        rc = L.cls_reach_diff(eng.h, C.byref(spec), _ptr(base), C.byref(out), _abi.F_DEVICE, None)
        assert rc == 0, L.cls_last_error(eng.h)

    def bound(name):
        return [i for i in ifs if bind[i][0] == name], [i for i in ifs if bind[i][1] == name]
    # the baseline: one local ACL deleted, one re-put with other rules; then the set as it was
    gone, reput = "local4", "local9"
    matrix()
    sync()
    first = dv.clone()
    assert eng.acl_del(gone) == 0
    assert eng.acl_put(reput, (random_acl16 if a.af == 16 else random_acl)(7001, 40, weird=0.0)[0], *bound(reput)) == 0
    matrix(base)
    sync()
    for name in (gone, reput):
        assert eng.acl_put(name, by_name[name], *bound(name)) == 0
    matrix()
    sync()
    assert torch.equal(dv, first), "the ACL set was not restored"
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(piped(matrix, a.iters, sync))
        tb.append(piped(diff, a.iters, sync))
    # parity: the new matrix, the total and the records against a compare of the two matrices
    sync()
    assert torch.equal(dv, first), "cls_reach_diff's matrix differs from cls_reach_matrix's"
    cell = torch.nonzero(base != dv).flatten()
    n_changed = int(total[0])
    assert n_changed == cell.numel(), (n_changed, cell.numel())
    k = min(n_changed, DIFF_CAP)
    r = rec[:k].to(torch.int64)
    assert torch.equal((r[:, 0] * n + r[:, 1]) * n + r[:, 2], cell[:k]), "records out of cell order"
    assert torch.equal(r[:, 3] & 0xFF, base[cell[:k]].to(torch.int64)) and \
        torch.equal(r[:, 3] >> 8, dv[cell[:k]].to(torch.int64))
    assert int(trans.sum()) == cells and int(changed.sum()) == n_changed
    t_a, t_b = float(np.median(ta)), float(np.median(tb))
    line = {"metric": "reachability diff: B / A (cls_reach_diff(CLS_F_DEVICE) with records (cap 1 Mi), total, "
                      "transitions and changed-per-row against cls_reach_matrix(CLS_F_DEVICE), the same three "
                      "matrix outputs, alternated in one process)",
            "af": a.af, "endpoints": n, "probes": N_PROBES, "cells": cells, "local_acls": n_local,
            "options": a.opt, "iters": a.iters, "rounds": a.rounds,
            "A_ms": round(t_a, 4), "B_ms": round(t_b, 4), "B_over_A": round(t_b / t_a, 4),
            "A_ms_rounds": [round(x, 4) for x in ta], "B_ms_rounds": [round(x, 4) for x in tb],
            "changed_cells": n_changed,
            "parity": "matrix == cls_reach_matrix's; total, record order, was / now == compare of the two matrices"}
    eng.close()
    return line


PORTS_MAX_ROWS = 1 << 32


def measure_ports(a, n_local):
    """A / B of cls_reach_matrix at the class starts and cls_reach_ports."""
    import torch
    from vpp_amd import _abi
    from vpp_amd.engine import Engine, _ptr
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    proto, sport = 0, 40000
    bind, by_name, ifs, at, addrs, _ = setup(eng, a.af, n_local, 2048)
    # the classes over all interfaces' ACLs: what 2048 endpoints on every interface bind
    names = sorted({x for i in np.unique(at) for x in bind[ifs[i]] if x is not None})
    starts = np.unique(np.concatenate([eng.port_classes(by_name[x], proto) for x in names]))
    K = len(starts)
    n = max([m for m in (2048, 1024, 512, 256) if K * m * m <= PORTS_MAX_ROWS] or [256])
    at, addrs = at[:n], addrs[:n]
    names_n = sorted({x for i in np.unique(at) for x in bind[ifs[i]] if x is not None})
    assert names_n == names, "the first N endpoints bind fewer ACLs"
    ids = np.array([eng.if_id(x) for x in ifs], np.uint32)
    rows = K * n * n
    L, sync = _abi.lib(), torch.cuda.synchronize
    ep_if = np.ascontiguousarray(ids[at], np.uint32)
    ep_addr = np.ascontiguousarray(addrs, np.uint8 if a.af == 16 else np.uint32)
    pr, sp = np.full(K, proto, np.uint8), np.full(K, sport, np.uint16)
    dp = starts.astype(np.uint16)
    spec_a = _abi.ReachSpec(a.af, n, _ptr(ep_if), None if a.af == 16 else _ptr(ep_addr),
                            _ptr(ep_addr) if a.af == 16 else None, K, _ptr(pr), _ptr(sp), _ptr(dp))
    spec_b = _abi.ReachSpec(a.af, n, _ptr(ep_if), None if a.af == 16 else _ptr(ep_addr),
                            _ptr(ep_addr) if a.af == 16 else None, 1, _ptr(pr), _ptr(sp), None)
    dv = torch.empty(rows, dtype=torch.uint8, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    runs = torch.empty((n, n), dtype=torch.int32, device="cuda")
    allow = torch.empty((n, n), dtype=torch.int32, device="cuda")
    hist = torch.empty(4, dtype=torch.int64, device="cuda")
    k_out = np.zeros(1, np.uint32)
    # the ranges are counted first: the cap of the timed calls is their total
    o = _abi.ReachPortsOut(None, 0, _ptr(total), None, None, None, _ptr(k_out))
    assert L.cls_reach_ports(eng.h, C.byref(spec_b), C.byref(o), _abi.F_DEVICE, None) == 0, L.cls_last_error(eng.h)
    sync()
    n_ranges = int(total[0])
    assert int(k_out[0]) == K, (int(k_out[0]), K)
    rec = torch.empty((n_ranges, 4), dtype=torch.int32, device="cuda")
    o = _abi.ReachPortsOut(_ptr(rec), n_ranges, _ptr(total), _ptr(runs), _ptr(allow), _ptr(hist), _ptr(k_out))

    def matrix():
        rc = L.cls_reach_matrix(eng.h, C.byref(spec_a), _ptr(dv), None, None, _abi.F_DEVICE, None)
        assert rc == 0, L.cls_last_error(eng.h)

    def ports():
        rc = L.cls_reach_ports(eng.h, C.byref(spec_b), C.byref(o), _abi.F_DEVICE, None)
        assert rc == 0, L.cls_last_error(eng.h)
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(piped(matrix, a.iters, sync))
        tb.append(piped(ports, a.iters, sync))
    # parity on the device: A's verdicts, [K, N, N], run-length encoded per pair
    sync()
    v = dv.view(K, n * n)
    want_runs = torch.ones(n * n, dtype=torch.int64, device="cuda")
    width = torch.from_numpy(np.diff(np.append(starts.astype(np.int64), 65536))).to("cuda")
    want_allow = torch.zeros(n * n, dtype=torch.int64, device="cuda")
    want_hist = torch.zeros(4, dtype=torch.int64, device="cuda")
    for k in range(K):
        if k:
            want_runs += v[k] != v[k - 1]
        want_allow += (v[k] == 2) * width[k]
        want_hist += torch.bincount(v[k].to(torch.int64), minlength=4) * width[k]
    assert torch.equal(runs.flatten().to(torch.int64), want_runs), "runs differ from the matrix at the class starts"
    assert torch.equal(allow.flatten().to(torch.int64), want_allow) and torch.equal(hist, want_hist)
    assert int(total[0]) == n_ranges == int(want_runs.sum())
    r = rec.to(torch.int64)
    pair = r[:, 0] * n + r[:, 1]
    assert bool((pair[1:] >= pair[:-1]).all()) and torch.equal(torch.bincount(pair, minlength=n * n), want_runs)
    t_a, t_b = float(np.median(ta)), float(np.median(tb))
    line = {"metric": "port sweep: B / A (cls_reach_ports(CLS_F_DEVICE) with ranges, total, runs, ALLOW ports and "
                      "histogram against cls_reach_matrix(CLS_F_DEVICE, verdicts) with K probes at the class starts, "
                      "alternated in one process)",
            "af": a.af, "endpoints": n, "endpoints_rule": "largest of 2048, 1024, 512, 256 with K N^2 <= 2^32",
            "K": K, "rows": rows, "local_acls": n_local, "acls_bound": len(names),
            "options": a.opt, "iters": a.iters, "rounds": a.rounds,
            "A_ms": round(t_a, 4), "B_ms": round(t_b, 4), "B_over_A": round(t_b / t_a, 4),
            "A_ms_rounds": [round(x, 4) for x in ta], "B_ms_rounds": [round(x, 4) for x in tb],
            "ranges": n_ranges, "ranges_per_pair_max": int(want_runs.max()),
            "A_bytes_out": rows, "B_bytes_out": n_ranges * 16 + 2 * n * n * 4 + 40,
            "verdict_cells": hist.cpu().numpy().tolist(),
            "parity": "runs, ALLOW ports, histogram, total and the records' pairs == run-length of A's verdicts"}
    eng.close()
    return line


def reach_tile_of(a):
    """The engine's reach_tile under --opt: the default 16 Mi, or the option
    rounded up to a multiple of 1024 as the engine rounds it."""
    opts = dict(o.split("=", 1) for o in a.opt)
    return (int(opts["reach_tile"]) + 1023) & ~1023 if opts.get("reach_tile") else 16 << 20


def measure_external(a, n_local):
    """A / B of cls_connect_batch over the sweep's rows prebuilt in HBM and
    cls_reach_external."""
    import torch
    from vpp_amd import _abi
    from vpp_amd.engine import Engine, _ptr
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    n, P, D = 2048, N_PROBES, 2
    bind, by_name, ifs, at, addrs, (pr, sp, dp) = setup(eng, a.af, n_local, n)
    ext_name = ifs[0]                                   # bound to the global table both ways
    # the classes over the ACLs of the endpoints' interfaces and the remote one
    names = sorted({x for i in np.unique(at) for x in bind[ifs[i]] if x is not None} |
                   {x for x in bind[ext_name] if x is not None})
    starts = np.unique(np.concatenate([eng.addr_classes(by_name[x]) for x in names])).astype(np.int64)
    K = len(starts)
    ids = np.array([eng.if_id(x) for x in ifs], np.uint32)
    ext = int(eng.if_id(ext_name))
    lines, rows = D * P * n, D * P * n * K
    L, sync = _abi.lib(), torch.cuda.synchronize
    ep_if = np.ascontiguousarray(ids[at], np.uint32)
    ep_addr = np.ascontiguousarray(addrs, np.uint8 if a.af == 16 else np.uint32)
    spec = _abi.ReachSpec(a.af, n, _ptr(ep_if), None if a.af == 16 else _ptr(ep_addr),
                          _ptr(ep_addr) if a.af == 16 else None, P, _ptr(pr), _ptr(sp), _ptr(dp))
    # A's rows, line-major, built on the device
    dev = lambda x, t: torch.from_numpy(np.ascontiguousarray(x).view(t)).to("cuda")
    line = torch.arange(lines, device="cuda")
    ing = (line // (P * n) == 1)[:, None]
    pi, si = line // n % P, line % n
    t_if = dev(ep_if, np.int32)[si][:, None]
    ext_t = torch.full((1, 1), ext, dtype=torch.int32, device="cuda")
    full = lambda x: x.expand(lines, K).contiguous().view(-1)
    src_if, dst_if = full(torch.where(ing, ext_t, t_if)), full(torch.where(ing, t_if, ext_t))
    if a.af == 16:
        rem = np.zeros((K, 16), np.uint8)
        rem[:, 10:12] = 0xFF
        rem[:, 12:] = starts.astype(">u4").view(np.uint8).reshape(-1, 4)
        pod, rem, sel = dev(ep_addr, np.uint8)[si][:, None, :], dev(rem, np.uint8)[None], ing[:, :, None]
        shape = (lines, K, 16)
    else:
        pod, rem, sel = dev(ep_addr, np.int32)[si][:, None], dev(starts.astype(np.uint32), np.int32)[None], ing
        shape = (lines, K)
    src = torch.where(sel, rem, pod).expand(shape).contiguous().view(-1)
    dst = torch.where(sel, pod, rem).expand(shape).contiguous().view(-1)
    t_pr = full(dev(pr, np.uint8)[pi][:, None])
    t_sp, t_dp = full(dev(sp, np.int16)[pi][:, None]), full(dev(dp, np.int16)[pi][:, None])
    cv = torch.empty(rows, dtype=torch.uint8, device="cuda")
    asz = 16 if a.af == 16 else 1
    per = max(1, reach_tile_of(a) // K) * K              # whole lines, as B's tiles
    batches = []
    for f in range(0, rows, per):
        cnt = min(per, rows - f)
        sl = (src[f * asz:(f + cnt) * asz], dst[f * asz:(f + cnt) * asz], t_sp[f:f + cnt], t_dp[f:f + cnt],
              t_pr[f:f + cnt], src_if[f:f + cnt], dst_if[f:f + cnt])
        if a.af == 16:
            pk = _abi.PktSoa(_abi.AF_V16, None, None, _ptr(sl[0]), _ptr(sl[1]), _ptr(sl[2]), _ptr(sl[3]), _ptr(sl[4]))
        else:
            pk = _abi.PktSoa(_abi.AF_V4, _ptr(sl[0]), _ptr(sl[1]), None, None, _ptr(sl[2]), _ptr(sl[3]), _ptr(sl[4]))
        batches.append((_abi.ConnSoa(pk, _ptr(sl[5]), _ptr(sl[6])), cnt, cv.data_ptr() + f, sl))
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    runs = torch.empty((D, P, n), dtype=torch.int32, device="cuda")
    allow = torch.empty((D, P, n), dtype=torch.int64, device="cuda")
    hist = torch.empty((D, P, 4), dtype=torch.int64, device="cuda")
    k_out = np.zeros(1, np.uint32)
    fn = L.cls_reach_external
    # the ranges are counted first: the cap of the timed calls is their total
    o = _abi.ReachExtOut(None, 0, _ptr(total), None, None, None, _ptr(k_out))
    assert fn(eng.h, C.byref(spec), ext, 3, C.byref(o), _abi.F_DEVICE, None) == 0, L.cls_last_error(eng.h)
    sync()
    n_ranges = int(total[0])
    assert int(k_out[0]) == K, (int(k_out[0]), K)
    rec = torch.empty((n_ranges, 4), dtype=torch.int32, device="cuda")
    o = _abi.ReachExtOut(_ptr(rec), n_ranges, _ptr(total), _ptr(runs), _ptr(allow), _ptr(hist), _ptr(k_out))

    def connect():
        for cs, cnt, out, _ in batches:
            assert L.cls_connect_batch(eng.h, C.byref(cs), cnt, out, _abi.F_DEVICE, None) == 0

    def external():
        assert fn(eng.h, C.byref(spec), ext, 3, C.byref(o), _abi.F_DEVICE, None) == 0, L.cls_last_error(eng.h)
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(piped(connect, a.iters, sync))
        tb.append(piped(external, a.iters, sync))
    # parity on the device: A's verdicts, [lines, K], run-length encoded per line
    sync()
    v = cv.view(lines, K)
    first = torch.ones((lines, K), dtype=torch.bool, device="cuda")
    first[:, 1:] = v[:, 1:] != v[:, :-1]
    want_runs = first.sum(dim=1)
    width = torch.from_numpy(np.diff(np.append(starts, 1 << 32))).to("cuda")
    want_allow = ((v == 2) * width[None]).sum(dim=1)
    want_hist = torch.stack([((v == x) * width[None]).sum(dim=1).view(D * P, n).sum(dim=1) for x in range(4)], dim=1)
    assert torch.equal(runs.flatten().to(torch.int64), want_runs), "runs differ from the batch at the class starts"
    assert torch.equal(allow.flatten(), want_allow) and torch.equal(hist.view(D * P, 4), want_hist)
    assert int(total[0]) == n_ranges == int(want_runs.sum())
    li, ki = first.nonzero(as_tuple=True)                # row-major: (line, class) ascending
    st = torch.from_numpy(starts).to("cuda")
    last = torch.ones(len(li), dtype=torch.bool, device="cuda")
    last[:-1] = li[1:] != li[:-1]
    hi = torch.full((len(li),), (1 << 32) - 1, dtype=torch.int64, device="cuda")
    hi[:-1] = torch.where(last[:-1], hi[:-1], st[ki[1:]] - 1)
    want_rec = torch.stack([li % n, (li // n % P) | (li // (P * n)) << 16 | v[li, ki].to(torch.int64) << 24, st[ki], hi],
                           dim=1)
    assert torch.equal(rec.to(torch.int64) & 0xFFFFFFFF, want_rec), "records differ from the batch's run lengths"
    t_a, t_b = float(np.median(ta)), float(np.median(tb))
    out = {"metric": "external sweep: B / A (cls_reach_external(CLS_F_DEVICE) with ranges, total, runs, ALLOW "
                     "addresses and histogram against cls_connect_batch(CLS_F_DEVICE) over the same D P N K rows "
                     "prebuilt in HBM, alternated in one process)",
           "af": a.af, "endpoints": n, "probes": P, "directions": D, "K": K, "rows": rows, "local_acls": n_local,
           "acls_bound": len(names), "ext_if": ext_name, "options": a.opt, "iters": a.iters, "rounds": a.rounds,
           "A_ms": round(t_a, 4), "B_ms": round(t_b, 4), "B_over_A": round(t_b / t_a, 4),
           "A_ms_rounds": [round(x, 4) for x in ta], "B_ms_rounds": [round(x, 4) for x in tb],
           "ranges": n_ranges, "ranges_per_line_max": int(want_runs.max()),
           "A_bytes_out": rows, "A_bytes_in_hbm": rows * (2 * (16 if a.af == 16 else 4) + 13),
           "B_bytes_out": n_ranges * 16 + lines * 12 + D * P * 32 + 8,
           "verdict_addresses": hist.view(D * P, 4).sum(dim=0).cpu().numpy().tolist(),
           "parity": "runs, ALLOW addresses, histogram, total and every record == run-length of A's verdicts"}
    eng.close()
    return out


HOPS_SYNTH_N = 8192


def measure_hops(a, n, n_local):
    """A / B of cls_reach_matrix and cls_reach_hops on the same engine."""
    import torch
    import reach_hops_cases as hc
    from vpp_amd import _abi
    from vpp_amd.engine import Engine, _ptr
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    bind, by_name, ifs, at, addrs, (pr, sp, dp) = setup(eng, a.af, n_local, n)
    ids = np.array([eng.if_id(x) for x in ifs], np.uint32)
    cells = N_PROBES * n * n
    L, sync = _abi.lib(), torch.cuda.synchronize
    ep_if = np.ascontiguousarray(ids[at], np.uint32)
    ep_addr = np.ascontiguousarray(addrs, np.uint8 if a.af == 16 else np.uint32)
    spec = _abi.ReachSpec(a.af, n, _ptr(ep_if), None if a.af == 16 else _ptr(ep_addr),
                          _ptr(ep_addr) if a.af == 16 else None, N_PROBES, _ptr(pr), _ptr(sp), _ptr(dp))
    dv = torch.empty(cells, dtype=torch.uint8, device="cuda")
    dh = torch.empty((N_PROBES, 4), dtype=torch.int64, device="cuda")
    da = torch.empty((N_PROBES, n), dtype=torch.int32, device="cuda")
    hops = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    reach = torch.empty(n, dtype=torch.int32, device="cuda")
    levels = torch.empty(256, dtype=torch.int64, device="cuda")
    out = _abi.ReachHopsOut(_ptr(hops), _ptr(reach), None, _ptr(levels), None)

    def matrix():
        rc = L.cls_reach_matrix(eng.h, C.byref(spec), _ptr(dv), _ptr(dh), _ptr(da), _abi.F_DEVICE, None)
        assert rc == 0, L.cls_last_error(eng.h)

    def closure():
        rc = L.cls_reach_hops(eng.h, C.byref(spec), None, 0, C.byref(out), _abi.F_DEVICE, None)
        assert rc == 0, L.cls_last_error(eng.h)
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(piped(matrix, a.iters, sync))
        tb.append(piped(closure, a.iters, sync))
    by_rows = {}
    if not a.child:
        for rows in (4, 8, 16):
            eng.set_option("hops_rows", rows)
            by_rows[str(rows)] = round(float(np.median([piped(closure, a.iters, sync) for _ in range(3)])), 4)
        eng.set_option("hops_rows", None)
    # the host alternative, once: A's verdicts downloaded and searched on the CPU; B checked against it
    closure()
    sync()
    line = {"metric": "hop closure: B / A (cls_reach_hops(CLS_F_DEVICE) with hop counts, reach counts and the level "
                      "histogram against cls_reach_matrix(CLS_F_DEVICE) with verdicts, histogram and allow counts "
                      "over the same spec, alternated in one process)",
            "af": a.af, "endpoints": n, "probes": N_PROBES, "cells": cells, "local_acls": n_local,
            "options": a.opt, "iters": a.iters, "rounds": a.rounds}
    t_a, t_b = float(np.median(ta)), float(np.median(tb))
    line.update({"A_ms": round(t_a, 4), "B_ms": round(t_b, 4), "B_over_A": round(t_b / t_a, 4),
                 "A_ms_rounds": [round(x, 4) for x in ta], "B_ms_rounds": [round(x, 4) for x in tb],
                 "B_ms_by_hops_rows": by_rows})
    if not a.child:
        t0 = time.perf_counter()
        v = dv.cpu().numpy().reshape(N_PROBES, n, n)
        t1 = time.perf_counter()
        want = hc.hops_ref(hc.adjacency(v))
        t2 = time.perf_counter()
        got = hops.cpu().numpy()
        assert np.array_equal(got, want), "cls_reach_hops differs from hops_ref of cls_reach_matrix's verdicts"
        w_reach, _, w_levels, _ = hc.sums(want)
        assert np.array_equal(reach.cpu().numpy().view(np.uint32), w_reach)
        assert np.array_equal(levels.cpu().numpy().view(np.uint64), w_levels)
        line.update({"CPU_download_ms": round((t1 - t0) * 1e3, 2), "CPU_hops_ref_ms": round((t2 - t1) * 1e3, 2),
                     "CPU_note": "the host alternative, measured once on the CPU: A's %d verdict bytes downloaded, "
                                 "then the numpy level-synchronous search" % cells,
                     "levels": {str(k): int(c) for k, c in enumerate(w_levels) if c},
                     "A_bytes_out": cells, "B_bytes_out": n * n + n * 4 + 256 * 8,
                     "parity": "hop counts, reach counts and levels == hops_ref / sums of A's verdicts"})
    eng.close()
    return line


def measure_hops_matrix(a):
    """The matrix form at N = 8192 on a synthetic random device matrix."""
    import torch
    from vpp_amd import _abi
    from vpp_amd.engine import Engine, _ptr
    n = HOPS_SYNTH_N
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    L, sync = _abi.lib(), torch.cuda.synchronize
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    m = torch.where(torch.rand((n, n), device="cuda", generator=g) < 2.0 / n, 2, 0).to(torch.uint8).contiguous()
    spec = _abi.ReachSpec(_abi.AF_V4, n, None, None, None, 1, None, None, None)
    hops = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    reach = torch.empty(n, dtype=torch.int32, device="cuda")
    levels = torch.empty(256, dtype=torch.int64, device="cuda")
    out = _abi.ReachHopsOut(_ptr(hops), _ptr(reach), None, _ptr(levels), None)

    def closure():
        rc = L.cls_reach_hops(eng.h, C.byref(spec), _ptr(m), 0, C.byref(out), _abi.F_DEVICE, None)
        assert rc == 0, L.cls_last_error(eng.h)
    t = [piped(closure, 3, sync) for _ in range(3)]
    by_rows = {}
    for rows in (4, 8, 16):
        eng.set_option("hops_rows", rows)
        by_rows[str(rows)] = round(float(np.median([piped(closure, 3, sync) for _ in range(3)])), 4)
    eng.set_option("hops_rows", None)
    closure()
    sync()
    # parity: a queue search from 64 sources over the adjacency lists
    adj = (m == 2).cpu().numpy()
    np.fill_diagonal(adj, False)
    nbr = [np.flatnonzero(r) for r in adj]
    got = hops.cpu().numpy()
    for s in np.random.default_rng(3).choice(n, 64, replace=False):
        dist = np.full(n, 255, np.int64)
        dist[s] = 0
        front = [int(s)]
        for level in range(1, 255):
            nxt = []
            for u in front:
                for v in nbr[u]:
                    if dist[v] == 255:
                        dist[v] = level
                        nxt.append(int(v))
            front = nxt
            if not front:
                break
        assert np.array_equal(got[s], dist.astype(np.uint8)), "source %d differs from the queue search" % s
    lv = levels.cpu().numpy()
    assert int(lv[0]) == n and int(lv.sum()) == n * n
    line = {"metric": "hop closure, matrix form: cls_reach_hops(CLS_F_DEVICE) over a synthetic random [1, N, N] device "
                      "matrix of out-degree about 2, with hop counts, reach counts and the level histogram",
            "endpoints": n, "edges": int(adj.sum()), "options": a.opt, "ms": round(float(np.median(t)), 4),
            "ms_rounds": [round(x, 4) for x in t], "ms_by_hops_rows": by_rows, "deepest_level": int(np.flatnonzero(lv[:255]).max()),
            "unreached_pairs": int(lv[255]), "parity": "64 sources == a queue search on the host"}
    eng.close()
    return line


def measure_classes(a, n, n_local):
    """A / B of cls_reach_matrix and cls_reach_classes on the same engine, and
    the matrix form over A's device matrix against the host alternative."""
    import torch
    import reach_classes_cases as cc
    from vpp_amd import _abi
    from vpp_amd.engine import Engine, _ptr, expand_classes
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    bind, by_name, ifs, at, addrs, (pr, sp, dp) = setup(eng, a.af, n_local, n)
    ids = np.array([eng.if_id(x) for x in ifs], np.uint32)
    cells = N_PROBES * n * n
    L, sync = _abi.lib(), torch.cuda.synchronize
    ep_if = np.ascontiguousarray(ids[at], np.uint32)
    ep_addr = np.ascontiguousarray(addrs, np.uint8 if a.af == 16 else np.uint32)
    spec = _abi.ReachSpec(a.af, n, _ptr(ep_if), None if a.af == 16 else _ptr(ep_addr),
                          _ptr(ep_addr) if a.af == 16 else None, N_PROBES, _ptr(pr), _ptr(sp), _ptr(dp))
    dv = torch.empty(cells, dtype=torch.uint8, device="cuda")
    dv2 = torch.empty(cells, dtype=torch.uint8, device="cuda")
    dh = torch.empty((N_PROBES, 4), dtype=torch.int64, device="cuda")
    da = torch.empty((N_PROBES, n), dtype=torch.int32, device="cuda")
    cap = 1024
    classes = torch.empty(n, dtype=torch.int32, device="cuda")
    reps = torch.empty(cap, dtype=torch.int32, device="cuda")
    sizes = torch.empty(cap, dtype=torch.int32, device="cuda")
    self_ = torch.empty(N_PROBES * cap, dtype=torch.uint8, device="cuda")
    quot = torch.empty(N_PROBES * cap * cap, dtype=torch.uint8, device="cuda")
    count, rounds = np.zeros(1, np.uint32), np.zeros(1, np.uint32)

    def out(verdict):
        return _abi.ReachClassesOut(_ptr(classes), _ptr(count), cap, _ptr(reps), _ptr(sizes), _ptr(self_), _ptr(quot),
                                    verdict, _ptr(rounds), None)
    o_plain, o_verdict = out(None), out(_ptr(dv2))

    def matrix():
        rc = L.cls_reach_matrix(eng.h, C.byref(spec), _ptr(dv), _ptr(dh), _ptr(da), _abi.F_DEVICE, None)
        assert rc == 0, L.cls_last_error(eng.h)

    def call(o, m=None):
        def f():
            rc = L.cls_reach_classes(eng.h, C.byref(spec), m, C.byref(o), _abi.F_DEVICE, None)
            assert rc == 0, L.cls_last_error(eng.h)
        return f
    b_plain, b_verdict, b_matrix = call(o_plain), call(o_verdict), call(o_plain, _ptr(dv))
    ta, tb, tv, tm = [], [], [], []
    for _ in range(a.rounds):
        ta.append(piped(matrix, a.iters, sync))
        tb.append(piped(b_plain, a.iters, sync))
        tv.append(piped(b_verdict, a.iters, sync))
        tm.append(piped(b_matrix, a.iters, sync))
    b_plain()
    k = int(count[0])
    assert k <= cap and int(rounds[0]) == 1, (k, int(rounds[0]))
    line = {"metric": "reachability classes: B / A (cls_reach_classes(CLS_F_DEVICE), evaluating form, with classes, "
                      "reps, sizes, self and quotient against cls_reach_matrix(CLS_F_DEVICE) with verdicts, histogram "
                      "and allow counts over the same spec, alternated in one process; B returns complete, A is "
                      "queued back to back)",
            "af": a.af, "endpoints": n, "probes": N_PROBES, "cells": cells, "local_acls": n_local,
            "options": a.opt, "iters": a.iters, "rounds": a.rounds, "lib": os.path.basename(_abi.LIB_PATH)}
    med = lambda t: round(float(np.median(t)), 4)
    line.update({"A_ms": med(ta), "B_ms": med(tb), "B_over_A": round(med(tb) / med(ta), 4),
                 "B_with_device_verdict_ms": med(tv), "matrix_form_ms": med(tm),
                 "A_ms_rounds": [round(x, 4) for x in ta], "B_ms_rounds": [round(x, 4) for x in tb],
                 "classes": k, "rounds_taken": int(rounds[0]),
                 "A_bytes_out": cells, "B_bytes_out": n * 4 + k * 8 + N_PROBES * k * (k + 1)})
    if not a.child:
        # the host alternative, once: A's matrix downloaded and grouped with numpy; B checked against it
        matrix()
        sync()
        t0 = time.perf_counter()
        v = dv.cpu().numpy().reshape(N_PROBES, n, n)
        t1 = time.perf_counter()
        want = cc.classes_ref(v)
        t2 = time.perf_counter()
        got = (classes.cpu().numpy().view(np.uint32), reps.cpu().numpy().view(np.uint32)[:k],
               sizes.cpu().numpy().view(np.uint32)[:k], self_.cpu().numpy()[:N_PROBES * k].reshape(N_PROBES, k),
               quot.cpu().numpy()[:N_PROBES * k * k].reshape(N_PROBES, k, k))
        for g, w in zip(got, want):
            assert np.array_equal(g, w), "cls_reach_classes differs from classes_ref of cls_reach_matrix's verdicts"
        assert np.array_equal(expand_classes(got[0], got[3], got[4]), v)
        b_verdict()
        assert np.array_equal(dv2.cpu().numpy().reshape(v.shape), v)
        # the host share of B: the same pipeline on the host over the downloaded matrix, and its grouping alone
        t3 = time.perf_counter()
        eng.reach_classes(None, None, None, None, None, matrix=v, class_cap=cap)
        t4 = time.perf_counter()
        line.update({"CPU_download_ms": round((t1 - t0) * 1e3, 2), "CPU_classes_ref_ms": round((t2 - t1) * 1e3, 2),
                     "host_matrix_form_ms": round((t4 - t3) * 1e3, 2),
                     "CPU_note": "the host alternative, measured once on the CPU: A's %d verdict bytes downloaded, then "
                                 "the tests' numpy grouping; host_matrix_form_ms: the call over that host matrix" % cells,
                     "class_sizes_top": sorted(want[2].tolist(), reverse=True)[:8],
                     "parity": "classes, reps, sizes, self, quotient == classes_ref of A's verdicts; "
                               "expand_classes == A's verdicts; verdict_out == A's verdicts"})
    eng.close()
    return line


def kernel_stats(a, n, diff_locals=None, ports=False, hops=False, classes=False, external=False):
    """The same measurement in a child under rocprofv3 --kernel-trace --stats
    (a run of its own: the timings above are taken without the profiler):
    average ns per call of the matrix's kernels and of connect_kernel
    (diff_locals: of the --diff measurement at that many local ACLs, with the
    diff's kernels)."""
    with tempfile.TemporaryDirectory() as d:
        mode = ["--locals", str(a.locals), "--tiles", str(a.stats_tile), "--cpu-sample", "256"]
        if diff_locals is not None:
            mode = ["--external" if external else "--classes" if classes else "--hops" if hops else "--ports" if ports else "--diff", "--diff-locals", str(diff_locals), "--rounds", str(a.rounds)]
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--af", str(a.af), "--endpoints", str(n),
               "--iters", str(a.iters)] + mode + [x for o in a.opt for x in ("--opt", o)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": r.stderr[-400:]}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv"}
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row["Name"]
            for key in ("reach_expand4", "reach_expand16", "reach_reduce", "reach_diff_count", "reach_diff_scan",
                        "reach_diff_emit", "reach_ports_expand4", "reach_ports_expand16", "reach_ports_count",
                        "reach_ports_emit", "reach_adj_fold", "reach_hops_bfs", "reach_class_fold", "reach_class_verify",
                        "reach_ext_expand4", "reach_ext_expand16", "reach_ext_count", "reach_ext_emit",
                        "connect_kernel"):
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
    ap.add_argument("--diff", action="store_true", help="A / B of cls_reach_matrix and cls_reach_diff")
    ap.add_argument("--diff-locals", default="12,64")
    ap.add_argument("--ports", action="store_true", help="A / B of cls_reach_matrix at the class starts and "
                                                         "cls_reach_ports")
    ap.add_argument("--hops", action="store_true", help="A / B of cls_reach_matrix and cls_reach_hops")
    ap.add_argument("--classes", action="store_true", help="A / B of cls_reach_matrix and cls_reach_classes")
    ap.add_argument("--external", action="store_true", help="A / B of cls_connect_batch over the sweep's prebuilt rows "
                                                            "and cls_reach_external")
    ap.add_argument("--rounds", type=int, default=7, help="--diff, --ports, --hops, --classes, --external: "
                                                          "alternations of A and B")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE")
    a = ap.parse_args()
    a.tiles = [int(x) for x in a.tiles.split(",")]
    if a.external:
        for n_local in [int(x) for x in a.diff_locals.split(",")]:
            line = measure_external(a, n_local)
            if a.kernel_stats and not a.child:
                from vpp_amd import _abi
                ks = kernel_stats(a, line["endpoints"], n_local, external=True)
                # per 4 Mi rows: a launch takes a tile of whole lines, about reach_tile rows (the last one fewer)
                lines = line["rows"] // line["K"]
                per_launch = line["rows"] / -(-lines // max(1, reach_tile_of(a) // line["K"]))
                for key, e in ks.items():
                    if isinstance(e, dict) and "avg_us" in e:
                        e["us_per_4Mi_rows"] = round(e["avg_us"] * (4 << 20) / per_launch, 2)
                line["kernel_stats"] = dict(ks, sources=_abi.source_hash(),
                                            note="average per launch over the A and B calls, under the profiler; "
                                                 "per 4 Mi rows from the rows of an average launch (reach_diff_scan: "
                                                 "one workgroup per launch)")
            print(json.dumps(line), flush=True)
        return
    if a.classes:
        for n in [int(x) for x in (a.endpoints if a.endpoints != "1024,2048" else "2048").split(",")]:
            for n_local in [int(x) for x in a.diff_locals.split(",")]:
                line = measure_classes(a, n, n_local)
                if a.kernel_stats and not a.child:
                    from vpp_amd import _abi
                    line["kernel_stats"] = dict(kernel_stats(a, n, n_local, classes=True), sources=_abi.source_hash(),
                                                note="average per launch over the A and B calls, under the profiler")
                print(json.dumps(line), flush=True)
        return
    if a.hops:
        for n in [int(x) for x in (a.endpoints if a.endpoints != "1024,2048" else "2048").split(",")]:
            for n_local in [int(x) for x in a.diff_locals.split(",")]:
                line = measure_hops(a, n, n_local)
                if a.kernel_stats and not a.child:
                    from vpp_amd import _abi
                    line["kernel_stats"] = dict(kernel_stats(a, n, n_local, hops=True), sources=_abi.source_hash(),
                                                note="average per launch over the A and B calls, under the profiler")
                print(json.dumps(line), flush=True)
        if not a.child:
            print(json.dumps(measure_hops_matrix(a)), flush=True)
        return
    if a.ports:
        for n_local in [int(x) for x in a.diff_locals.split(",")]:
            line = measure_ports(a, n_local)
            if a.kernel_stats and not a.child:
                from vpp_amd import _abi
                ks = kernel_stats(a, line["endpoints"], n_local, ports=True)
                # per 4 Mi rows: a launch takes a tile, about reach_tile rows (the last one fewer)
                tile = 16 << 20
                b_rows = line["rows"] / -(-line["endpoints"] ** 2 // max(1, tile // line["K"]))
                a_rows = line["rows"] / -(-line["rows"] // tile)
                for key, e in ks.items():
                    if isinstance(e, dict) and "avg_us" in e:
                        per = b_rows if key.startswith("reach_ports") or key == "reach_diff_scan" else \
                            a_rows if key.startswith("reach_expand") else (a_rows + b_rows) / 2
                        e["us_per_4Mi_rows"] = round(e["avg_us"] * (4 << 20) / per, 2)
                line["kernel_stats"] = dict(ks, sources=_abi.source_hash(),
                                            note="average per launch over the A and B calls, under the profiler; "
                                                 "per 4 Mi rows from the rows of an average launch (reach_diff_scan: "
                                                 "one workgroup per launch)")
            print(json.dumps(line), flush=True)
        return
    if a.diff:
        for n in [int(x) for x in (a.endpoints if a.endpoints != "1024,2048" else "2048").split(",")]:
            for n_local in [int(x) for x in a.diff_locals.split(",")]:
                line = measure_diff(a, n, n_local)
                if a.kernel_stats and not a.child:
                    from vpp_amd import _abi
                    line["kernel_stats"] = dict(kernel_stats(a, n, n_local), sources=_abi.source_hash(),
                                                note="average per launch over the A and B calls, under the profiler")
                print(json.dumps(line), flush=True)
        return
    for n in [int(x) for x in a.endpoints.split(",")]:
        line = measure(a, n)
        if a.kernel_stats and not a.child:
            from vpp_amd import _abi
            line["kernel_stats"] = dict(kernel_stats(a, n), sources=_abi.source_hash(),
                                        tile=a.stats_tile, note="average per launch at this tile size, under the profiler")
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
