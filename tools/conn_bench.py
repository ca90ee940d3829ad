#!/usr/bin/env python3
"""Connection-path throughput (testConnection batches).

Layout: the config-3 global ACL (9963 rules) bound to if0/if1 (in) and
if0/if2 (out), 64 random local ACLs (1-300 rules) on 77 further interfaces,
half of the connections entering through a global-table interface.  Times
``Engine.connect_batch`` over N connections with host arrays in and out
(PCIe copies included; auto and linear modes) and with device-resident
tensors (CLS_F_DEVICE, ``hbm_resident``: the median wall time of --iters calls),
and the C oracle (one thread) on a sample.  Prints one JSON line.  --count 1 times CLS_F_COUNT batches (per-(ACL, rule) counters)
beside the plain ones; --locals sets the number of local ACLs (12: a rule
pool that fits LDS).
--af 16: the mixed-family layout (CLS_AF_V16) -- the config-5 table (IPv4 and
IPv6 networks) as the global ACL, random 16-byte local ACLs, endpoints of both
families (half of the connections from the config-5 stream, the others
around the locals' prefixes); the same line, 46 algorithmic bytes per
connection.  The connection stream floor is IPv4 only: the 16-byte line
reports the 16-byte classify stream's floor (35 B read, 1 B written per
packet) beside the 37 + 1 B of a pair launch (k16_pair.hip).
--trace: also times cls_connect_rules (the per-call matched-rule trace: 16 B
written per connection beside the verdict byte) on the same device batch, and
reports for the plain, the counted and the trace batch the GPU time of one
batch's launches (device events around a call on a stream of its own) beside
the back-to-back wall time -- "trace" in the JSON line; its rows are checked
against orc_test_connection_hits on the CPU sample.
usage: python tools/conn_bench.py [--n 4194304] [--iters 5] [--locals 64] [--af 4|16] [--trace]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from aclgen import random_acl16, random_traffic, random_traffic16  # noqa: E402
from test_gpu_connect_scale import build, oracle_connections  # noqa: E402


def build16(eng, seed, n_local, n_if=80):
    """build() of test_gpu_connect_scale for --af 16: the config-5 table as it
    is rendered (already both families) as the global ACL, random_acl16 locals."""
    import random

    from vpp_amd import workload
    rng = random.Random(seed)
    glob, spec, _ = workload.config(5)
    ifs = ["if%d" % i for i in range(n_if)]
    bind = {name: [None, None] for name in ifs}
    acls = [("global", glob.rules, ["if0", "if1"], ["if0", "if2"])]
    pool = None
    for k in range(n_local):
        size = rng.choice([1, 3, 12, 40, 150, 300])
        rules, pool = random_acl16(1000 + k, size, weird=rng.choice([0.0, 0.003, 0.15]))
        acls.append(("local%d" % k, rules, rng.sample(ifs[3:], rng.randrange(1, 3)),
                     rng.sample(ifs[3:], rng.randrange(0, 3))))
    by_name = {}
    for name, rules, ing, eg in acls:
        assert eng.acl_put(name, rules, ing, eg) == 0
        by_name[name] = rules
        for i in ing:
            bind[i][0] = name
        for i in eg:
            bind[i][1] = name
    return ifs, bind, by_name, pool, spec


def traffic16(n, pool, spec, half, rng):
    """Mixed-family endpoints: the config-5 stream where `half`, else
    addresses around the locals' prefixes (a base of 2^17 connections drawn
    with replacement: the address generator is per-address Python)."""
    import oracle
    base = random_traffic16(7, min(n, 1 << 17), pool)
    pick = rng.integers(0, len(base["proto"]), n)
    tr = {f: v[pick] for f, v in base.items()}
    g = oracle.gen_traffic_v16(spec, 0, n)
    for f in ("src", "dst", "dport", "proto"):
        tr[f][half] = g[f][half]
    return tr


def trace_times(a, eng, dargs, n):
    """--trace: the plain, counted and trace batch of the same device
    connections through the ABI on one build: ms per batch back to back (wall
    time over a.iters calls, one wait at the end) and the GPU time of one
    batch's launches (device events around each of a.iters calls on a stream
    of the tool's own; median)."""
    import ctypes as C

    import torch
    from vpp_amd import _abi
    from vpp_amd.engine import _ptr
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    rules = torch.full((n, 4), -2, dtype=torch.int32, device="cuda")
    if a.af == 16:
        pk = _abi.PktSoa(_abi.AF_V16, None, None, _ptr(dargs[2]), _ptr(dargs[3]), _ptr(dargs[5]), _ptr(dargs[6]),
                         _ptr(dargs[4]))
    else:
        pk = _abi.PktSoa(_abi.AF_V4, _ptr(dargs[2]), _ptr(dargs[3]), None, None, _ptr(dargs[5]), _ptr(dargs[6]),
                         _ptr(dargs[4]))
    cs = _abi.ConnSoa(pk, _ptr(dargs[0]), _ptr(dargs[1]))
    L, h, csr, op, rp = _abi.lib(), eng.h, C.byref(cs), _ptr(out), _ptr(rules)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    calls = {"plain": lambda s: L.cls_connect_batch(h, csr, n, op, _abi.F_DEVICE, s),
             "counted": lambda s: L.cls_connect_batch(h, csr, n, op, _abi.F_DEVICE | _abi.F_COUNT, s),
             "trace": lambda s: L.cls_connect_rules(h, csr, n, op, rp, _abi.F_DEVICE, s)}
    res = {}
    for kind, fn in calls.items():
        assert fn(None) == 0                                 # warm: the kind's plan and uploads
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            assert fn(None) == 0
        torch.cuda.synchronize()
        piped = (time.perf_counter() - t0) / a.iters
        assert fn(sp) == 0
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        for e0, e1 in evs:
            e0.record(stream)
            assert fn(sp) == 0
            e1.record(stream)
            stream.synchronize()
        res[kind] = {"abi_pipelined_ms_per_batch": round(piped * 1e3, 4),
                     "gpu_ms_per_batch": round(float(np.median([e0.elapsed_time(e1) for e0, e1 in evs])), 4)}
    res["bytes_written_per_connection"] = {"plain": 1, "counted": 1, "trace": 17}
    res["rows"] = rules.cpu().numpy()
    assert (res["rows"] >= -1).all()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--cpu-sample", type=int, default=20000, help="connections checked on the literal oracle")
    ap.add_argument("--cpu-fast-sample", type=int, default=1 << 20,
                    help="connections timed on the OpenMP fast port (the CPU baseline)")
    ap.add_argument("--other-proto", type=int, default=1, help="6%% of packets with protocol > 2")
    ap.add_argument("--locals", type=int, default=64)
    ap.add_argument("--count", type=int, default=1)
    ap.add_argument("--af", type=int, default=4, choices=[4, 16], help="16: mixed-family batches (CLS_AF_V16)")
    ap.add_argument("--trace", action="store_true", help="time cls_connect_rules beside the plain and counted batches")
    ap.add_argument("--no-check", action="store_true", help="diagnostic builds: skip the parity asserts")
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE",
                    help="library tuning switch (cls_engine_set_option), repeatable")
    a = ap.parse_args()
    from vpp_amd.engine import Engine
    eng = Engine(options=dict(o.split("=", 1) for o in a.opt))
    n = a.n
    rng = np.random.default_rng(7)
    half = rng.random(n) < 0.5
    if a.af == 16:
        ifs, bind, by_name, pool, spec = build16(eng, 0, a.locals)
        tr = traffic16(n, pool, spec, half, rng)
        if a.other_proto:                                # (the config-5 stream has none)
            oth = half & (rng.random(n) < 0.06)
            tr["proto"][oth] = 47
    else:
        ifs, bind, by_name, pool, spec = build(eng, 0, cfg=3, n_local=a.locals)
        tr = random_traffic(7, n, pool, other_proto=bool(a.other_proto))
        tr["src"][half] = rng.choice(spec["pod_ips"].astype(np.uint32), half.sum())
        dsts = spec["dst_addrs"].astype(np.uint32)
        tr["dst"][half] = rng.choice(dsts, half.sum()) | rng.integers(0, 256, half.sum()).astype(np.uint32)
    ids = np.array([eng.if_id(x) for x in ifs], np.uint32)
    si = np.where(half, rng.integers(0, 2, n), rng.integers(0, len(ifs), n))
    di = rng.integers(0, len(ifs), n)
    args = (ids[si], ids[di], tr["src"], tr["dst"], tr["proto"], tr["sport"], tr["dport"])
    res = {}
    for mode in ("linear", "auto"):
        out = eng.connect_batch(*args, mode=mode)        # warm-up (and table upload)
        t0 = time.perf_counter()
        for _ in range(a.iters):
            out = eng.connect_batch(*args, mode=mode)
        res[mode] = ((time.perf_counter() - t0) / a.iters, out)
    if not a.no_check:
        assert np.array_equal(res["linear"][1], res["auto"][1]), "linear and classifier modes differ"
    dt, out = res["auto"]
    # HBM-resident batch (CLS_F_DEVICE): no PCIe in the timed region
    import torch
    dargs = [torch.from_numpy(np.ascontiguousarray(x).view({4: np.int32, 2: np.int16, 1: np.uint8}[x.dtype.itemsize]))
             .to("cuda") for x in (args[0], args[1], args[2], args[3], args[4], args[5], args[6])]
    torch.cuda.synchronize()
    dev_out = eng.connect_batch(*dargs)
    if not a.no_check:
        assert np.array_equal(dev_out.cpu().numpy(), out), "device batch differs"
    vout = torch.empty(n, dtype=torch.uint8, device="cuda")

    def per_call(count):
        """median wall time of a.iters device batches, each waited for (the
        call is stream-ordered: it returns once its launches are queued), the
        verdicts into one output tensor"""
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            eng.connect_batch(*dargs, count=count, out=vout)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))
    dev_dt = per_call(False)

    def per_call_abi(count):
        """the same batch through cls_connect_batch with the call's arguments
        built once (what a native host pays: no per-call Python marshalling)"""
        import ctypes as C
        from vpp_amd import _abi
        from vpp_amd.engine import _ptr
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        if a.af == 16:
            pk = _abi.PktSoa(_abi.AF_V16, None, None, _ptr(dargs[2]), _ptr(dargs[3]), _ptr(dargs[5]), _ptr(dargs[6]),
                             _ptr(dargs[4]))
        else:
            pk = _abi.PktSoa(_abi.AF_V4, _ptr(dargs[2]), _ptr(dargs[3]), None, None, _ptr(dargs[5]), _ptr(dargs[6]),
                             _ptr(dargs[4]))
        cs = _abi.ConnSoa(pk, _ptr(dargs[0]), _ptr(dargs[1]))
        fl = _abi.F_DEVICE | (_abi.F_COUNT if count else 0)
        fn, h, csr, op = _abi.lib().cls_connect_batch, eng.h, C.byref(cs), _ptr(out)
        sync = torch.cuda.synchronize
        ts = []
        for _ in range(a.iters + 1):
            t0 = time.perf_counter()
            rc = fn(h, csr, n, op, fl, None)
            sync()
            ts.append(time.perf_counter() - t0)
            assert rc == 0
        # pipelined: a.iters batches queued back to back, one wait at the end
        # (the stream-ordered device batch: the host work of a call overlaps
        # the GPU work of the one before)
        t0 = time.perf_counter()
        for _ in range(a.iters):
            assert fn(h, csr, n, op, fl, None) == 0
        sync()
        piped = (time.perf_counter() - t0) / a.iters
        if not a.no_check:
            assert np.array_equal(out.cpu().numpy(), dev_out.cpu().numpy())
        return float(np.median(ts[1:])), piped
    abi_dt, abi_piped = per_call_abi(False)
    counted = None
    if a.count:
        eng.connect_batch(*dargs, count=True)
        dt_c = per_call(True)
        abi_c, abi_c_piped = per_call_abi(True)
        counted = {"value": round(n / dt_c / 1e6, 3), "unit": "Mconn/s", "ms_per_batch": round(dt_c * 1e3, 3),
                   "abi_ms_per_batch": round(abi_c * 1e3, 4),
                   "abi_pipelined_ms_per_batch": round(abi_c_piped * 1e3, 4)}
        # how the counted calls spread over the (ACL, rule) counters: the
        # shares of the largest counters (contention of the counter atomics)
        cs = np.concatenate([eng.conn_counters(name).astype(np.float64) for name in by_name])
        tot = cs.sum()
        top = np.sort(cs)[::-1][:8] / max(tot, 1.0)
        counted["calls_per_connection"] = round(tot / (n * (3 * a.iters + 2)), 3)
        counted["top_counter_shares"] = [round(float(x), 4) for x in top]
        counted["nonzero_counters"] = int((cs > 0).sum())
    # roofline: the 22 algorithmic bytes of an IPv4 connection (src, dst,
    # src_if, dst_if 4 B each, sport, dport 2 B, proto 1 B read; the verdict
    # byte written) per HBM-resident batch, beside the stream floor of the
    # same arrays (cls_stream_floor_conn: the same reads and write, no
    # evaluation)
    # (the product path: device batches through the C ABI, back to back)
    if a.af == 16:
        # 46 B: 16-B src and dst in place of the 4-B ones.  No connection
        # stream floor for this layout: the 16-byte classify stream's (35 B
        # read + 1 B written per packet), which a pair launch of one large ACL
        # (37 B read + 1 B written per connection) is measured against.
        floor = eng.stream_floor(dargs[2], dargs[3], dargs[6], dargs[4], vout, reps=20)
        roof = {"bound": "hbm", "bytes_per_connection": 46, "peak": 8000.0, "unit": "GB/s",
                "achieved": round(46 * n / abi_piped / 1e9, 1), "frac": round(46 * n / abi_piped / 8e12, 4),
                "classify16_stream_floor_ms": round(floor, 4), "classify16_stream_bytes": 36,
                "pair_launch_bytes": 38, "pair_launch_floor_ms": round(floor * 38 / 36, 4),
                "timed": "abi_pipelined_ms_per_batch"}
    else:
        floor = eng.stream_floor_conn(*dargs, reps=20)
        roof = {"bound": "hbm", "bytes_per_connection": 22, "peak": 8000.0, "unit": "GB/s",
                "achieved": round(22 * n / abi_piped / 1e9, 1), "frac": round(22 * n / abi_piped / 8e12, 4),
                "stream_floor_ms": round(floor, 4), "frac_of_stream_floor": round(floor / (abi_piped * 1e3), 4),
                "timed": "abi_pipelined_ms_per_batch"}
    trace = None
    if a.trace:
        trace = trace_times(a, eng, dargs, n)
    k = a.cpu_sample
    t1 = time.perf_counter()
    want, _ = oracle_connections(bind, by_name, ifs, si[:k], di[:k], {f: v[:k] for f, v in tr.items()}, a.af)
    cpu_dt = time.perf_counter() - t1
    if not a.no_check:
        assert np.array_equal(out[:k], want), "connection verdicts differ from the oracle"
    if trace is not None:
        rows = trace.pop("rows")
        if not a.no_check:
            from test_connect_trace_cpu import oracle_rows
            wv, wr = oracle_rows(bind, by_name, ifs, si[:k], di[:k], {f: v[:k] for f, v in tr.items()}, a.af)
            assert np.array_equal(wv, want) and np.array_equal(rows[:k], wr), "trace rows differ from the oracle"
            trace["parity"] = "first %d rows bit-exact vs orc_test_connection_hits" % k
    # the CPU baseline: the fast port (rules pre-parsed, orc_connect_fast)
    # over OpenMP on the cores this process may use, on a prefix of the batch
    import oracle
    from bench import cpu_share, host_cpu
    names = list(by_name)
    tabs = [oracle.FastTable(oracle.rules_to_c(by_name[x])) for x in names]
    if_ids = {x: i for i, x in enumerate(names)}
    if_in = [if_ids[bind[f][0]] if bind[f][0] else -1 for f in ifs]
    if_out = [if_ids[bind[f][1]] if bind[f][1] else -1 for f in ifs]
    kf = min(n, a.cpu_fast_sample)
    cores = cpu_share()
    trk = {f: v[:kf] for f, v in tr.items()}
    oracle.connect_fast(tabs, if_in, if_out, si[:1024], di[:1024], {f: v[:1024] for f, v in tr.items()},
                        af=a.af, nthreads=cores)
    t2 = time.perf_counter()
    fast = oracle.connect_fast(tabs, if_in, if_out, si[:kf], di[:kf], trk, af=a.af, nthreads=cores)
    fast_dt = time.perf_counter() - t2
    if not a.no_check:
        assert np.array_equal(fast, out[:kf]), "the fast CPU port differs from the GPU verdicts"
    print(json.dumps({
        "metric": "connections classified per second (testConnection, up to 4 ACL evaluations each)",
        "value": round(n / abi_piped / 1e6, 3), "unit": "Mconn/s", "n": n, "af": a.af,
        "ms_per_batch": round(abi_piped * 1e3, 4),
        "timed": "device batches through cls_connect_batch, back to back (HBM-resident, stream-ordered)",
        "host_arrays": {"value": round(n / dt / 1e6, 3), "unit": "Mconn/s", "ms_per_batch": round(dt * 1e3, 3),
                        "pcie_included": True},
        "global_rules": len(by_name["global"]), "local_acls": a.locals,
        "other_proto": bool(a.other_proto), "hbm_resident_counted": counted,
        "hbm_resident": {"value": round(n / dev_dt / 1e6, 3), "unit": "Mconn/s",
                         "ms_per_batch": round(dev_dt * 1e3, 4), "abi_ms_per_batch": round(abi_dt * 1e3, 4),
                         "abi_pipelined_ms_per_batch": round(abi_piped * 1e3, 4)},
        "roofline": roof, **({"trace": trace} if trace is not None else {}),
        "linear_scan": {"value": round(n / res["linear"][0] / 1e6, 3), "unit": "Mconn/s",
                        "ms_per_batch": round(res["linear"][0] * 1e3, 3)},
        "verdicts": np.bincount(out, minlength=4).tolist(),
        "cpu_baseline": {"value": round(kf / fast_dt / 1e6, 4), "unit": "Mconn/s", "cores": cores,
                         "kind": "port", "nproc": host_cpu()[0], "cpu_model": host_cpu()[1],
                         "sample": "%d connections of the batch, orc_connect_fast (ACLs pre-parsed, testConnection "
                                   "restated, OpenMP %d threads), %.1f s" % (kf, cores, fast_dt),
                         "faithful": {"value": round(k / cpu_dt / 1e6, 5), "unit": "Mconn/s", "cores": 1,
                                      "sample": "%d connections, orc_test_connection_hits (CIDR strings re-parsed "
                                                "per rule per call)" % k}},
        "parity": "first %d connections bit-exact vs oracle" % k}))
    eng.close()


if __name__ == "__main__":
    main()
