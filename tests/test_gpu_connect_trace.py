"""GPU: the connection trace (cls_connect_rules / Engine.connect_rules /
ACLEngine.connection_trace) against orc_test_connection_hits.

For every connection the trace gives the rule at which each of
testConnection's four evalACL calls ended (aclengine_mock.go:394-471; the
matched rule the reference logs, :651-654): the index in the call's ACL, R for
the default DENY, -1 for a call not made or made on a nil ACL.  Every case
here asserts

- the rows equal the oracle's hits[4] exactly,
- the verdicts equal the oracle's and cls_connect_batch's on the same inputs,
- the tables' connection counters (made non-zero by a counted batch first)
  are the same before and after the trace call,

over the paths the plan and the kernel can take: host and device batches with
every way of choosing large ACLs, odd batch sizes, the rule pool staged or
not, bitmap forms or scans, job lists or shuffles, counter-index words (u16,
u32) and slot words of the large ACLs from the pair launches or the slot
launches, two large ACLs (the early words), same-interface REFLECT, unknown
and unbound interfaces, guarded outputs, the kept device plan across batch
kinds and a binding change, a caller's stream, the renderer API and the Go
shims.  The workloads and their oracle rows come from
test_connect_trace_cpu.py (computed once per process), which also asserts on
the oracle alone that they exercise what is claimed.
"""
import os
import subprocess

import numpy as np
import pytest

from aclgen import random_acl
from test_connect_trace_cpu import LARGE_N_IF, WORKLOADS, Recorder, call_acls, oracle_rows, workload
from vpp_amd import _abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONNTRACE = os.path.join(ROOT, "go", "shimtest", "conntrace")


def _dev(x):
    import torch
    x = np.array(x, order="C")                        # (a copy: the shared workloads are read-only)
    if x.ndim == 2:
        return torch.from_numpy(x).to("cuda")
    return torch.from_numpy(x.view({4: np.int32, 2: np.int16, 1: np.uint8}[x.dtype.itemsize])).to("cuda")


def _engine(**opts):
    from vpp_amd.engine import Engine
    return Engine(options=opts or None)


def _args(eng, w, sel=None):
    """The workload's connections `sel` (default: all) as connect_batch's
    host arguments, with the engine's interface ids."""
    ids = np.array([eng.if_id(x) for x in w["ifs"]], np.uint32)
    tr = w["tr"]
    a = [ids[w["si"]], ids[w["di"]], tr["src"], tr["dst"], tr["proto"], tr["sport"], tr["dport"]]
    return a if sel is None else [x[sel] for x in a]


def _counters(eng, w):
    return {name: eng.conn_counters(name) for name in w["by_name"]}


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(want), max(1, want[:1].size)).any(1))[0]
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]].tolist(), want[bad[:8]].tolist())


def _check(eng, w, mode, device, sel=None, want=None):
    """One trace batch against the oracle rows, cls_connect_batch and the
    counters; returns (verdicts, rows) as numpy arrays."""
    want_v, want_r = want if want is not None else (w["verdict"], w["rows"])
    if sel is not None:
        want_v, want_r = want_v[sel], want_r[sel]
    args = _args(eng, w, sel)
    if device:
        import torch
        args = [_dev(x) for x in args]
        torch.cuda.synchronize()
    eng.connect_batch(*args, mode=mode, count=True)          # the counters: non-zero
    before = _counters(eng, w)
    assert sum(int(c.sum()) for c in before.values()) > 0 or len(want_v) == 0
    v, r = eng.connect_rules(*args, mode=mode)
    plain = eng.connect_batch(*args, mode=mode)
    if device:
        v, r, plain = v.cpu().numpy(), r.cpu().numpy(), plain.cpu().numpy()
    after = _counters(eng, w)
    assert r.dtype == np.int32 and r.shape == (len(want_v), 4) and v.dtype == np.uint8
    _same(r, want_r, "rules")
    _same(v, want_v, "verdict")
    _same(plain, want_v, "cls_connect_batch verdict")
    for name in before:
        assert np.array_equal(before[name], after[name]), name
    return v, r


# 20,003 connections for the device batches (no multiple of 4 or 64): the
# workload's 20,000 and its first three again
ODD = np.r_[0:20000, 0:3]
MODES = {"linear": ("linear", False), "classifier": ("classifier", False), "auto": ("auto", False),
         "device": ("classifier", True), "device_auto": ("auto", True)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("seed,fam,n_local", WORKLOADS)
def test_trace_matches_oracle_in_every_mode(seed, fam, n_local, mode):
    w = workload(seed, fam, n_local)
    eng = _engine()
    try:
        w["rec"].install(eng)
        m, device = MODES[mode]
        _check(eng, w, m, device, ODD if device else None)
    finally:
        eng.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("fam", [4, 16])
def test_batches_of_one_and_none(fam, device):
    w = workload(1, fam, 12)
    eng = _engine()
    try:
        w["rec"].install(eng)
        for sel in (np.r_[7:8], np.r_[0:0]):
            args = _args(eng, w, sel)
            if device:
                args = [_dev(x) for x in args]
            v, r = eng.connect_rules(*args, mode="classifier")
            if device:
                v, r = v.cpu().numpy(), r.cpu().numpy()
            assert r.shape == (len(sel), 4) and r.dtype == np.int32
            _same(r, w["rows"][sel], "rules")
            _same(v, w["verdict"][sel], "verdict")
    finally:
        eng.close()


@pytest.mark.parametrize("jobs", [1, 0])
@pytest.mark.parametrize("no_lds", [0, 2, 4])
@pytest.mark.parametrize("bitmap", [1, 0])
def test_pool_and_job_variants(bitmap, no_lds, jobs):
    """IPv4 at 64 local ACLs (a wave's jobs need more than one pass, so the
    never-made calls are dropped from the second packing): bitmap forms or
    scans, tables in LDS or global memory, LDS job lists or shuffles."""
    w = workload(0, 4, 64)
    eng = _engine(conn_bitmap=bitmap, conn_no_lds=no_lds, conn_jobs=jobs)
    try:
        w["rec"].install(eng)
        _check(eng, w, "auto", True, ODD)
    finally:
        eng.close()


def test_rule_pool_in_global_memory():
    """conn_no_lds bit 0: the rule pool read from global memory (the variants
    without the LDS-staged pool), IPv4 and 16-byte."""
    for fam in (4, 16):
        w = workload(1, fam, 12)
        eng = _engine(conn_no_lds=1)
        try:
            w["rec"].install(eng)
            _check(eng, w, "auto", True, ODD)
        finally:
            eng.close()


def _trace_lines(eng, w, capfd, mode="classifier"):
    """_check with the debug_conn lines of the trace batch alone."""
    args = _args(eng, w)
    eng.connect_batch(*args, mode=mode, count=True)
    before = _counters(eng, w)
    capfd.readouterr()
    v, r = eng.connect_rules(*args, mode=mode)
    err = capfd.readouterr().err.splitlines()
    _same(r, w["rows"], "rules")
    _same(v, w["verdict"], "verdict")
    _same(eng.connect_batch(*args, mode=mode), w["verdict"], "cls_connect_batch verdict")
    after = _counters(eng, w)
    for name in before:
        assert np.array_equal(before[name], after[name]), name
    return err


@pytest.mark.parametrize("opts,words", [({}, "u16"), ({"conn_pre_narrow": 0}, "u32"), ({"conn_pre_rules": 0}, "slots"),
                                        ({"conn_pair": 0}, "slot launches")])
def test_large_acl_words_ipv4(opts, words, capfd):
    """The global table (1003 rules, 3 of 24 interfaces) on the classifier:
    the pair launch's counter-index words as u16 or (conn_pre_narrow=0) u32
    -- never its one-byte result words, which carry no rule -- or
    (conn_pre_rules=0) its slot words, or (conn_pair=0) the two slot
    launches' words; the kernel takes the descriptor's counter base off the
    former and maps the latter through slot_rule."""
    w = workload(0, 4, 12, n_if=LARGE_N_IF)
    eng = _engine(debug_conn=1, **opts)
    try:
        w["rec"].install(eng)
        err = _trace_lines(eng, w, capfd)
    finally:
        eng.close()
    plan = [ln for ln in err if ln.startswith("connect:")]
    pimg = [ln for ln in err if ln.startswith("pair: pimg")]
    queue = [ln for ln in err if ln.startswith("pair:") and " o_at " in ln]
    assert len(plan) == 1 and " trace 1 " in plan[0] and " cmode 0 " in plan[0] and " ctr 0 " not in plan[0], plan
    assert " big 0 " not in plan[0], plan
    if words in ("u16", "u32"):
        assert pimg, err
        assert (" pre_rules 1 pre_bytes %d" % (2 if words == "u16" else 4)) in plan[0], plan
    elif words == "slots":
        assert queue and not pimg, err
        assert " pre_rules 0 pre_bytes 4" in plan[0], plan
    else:
        assert not pimg and not queue, err
        assert " pre_rules 0 pre_bytes 4" in plan[0], plan


@pytest.mark.parametrize("pair16", [1, 0])
def test_large_acl_words_16_byte(pair16, capfd):
    """16-byte batches: the pair launch on the pair image (counter-index
    words) or (conn_pair16=0) the two slot launches (slot words)."""
    w = workload(0, 16, 12, n_if=LARGE_N_IF)
    eng = _engine(debug_conn=1, conn_pair16=pair16)
    try:
        w["rec"].install(eng)
        err = _trace_lines(eng, w, capfd)
    finally:
        eng.close()
    plan = [ln for ln in err if ln.startswith("connect:")]
    pair = [ln for ln in err if ln.startswith("pair16:")]
    slots = [ln for ln in err if ln.startswith("slots16:")]
    assert len(plan) == 1 and " trace 1 " in plan[0] and " big 0 " not in plan[0], plan
    if pair16:
        assert pair and not slots, err
        assert " pre_rules 1 pre_bytes 2" in plan[0], plan
    else:
        assert slots and not pair, err
        assert " pre_rules 0 pre_bytes 4" in plan[0], plan


def test_two_large_acls(capfd):
    """Two large ACLs (the config-3 global table and a 3,000-rule random one
    on interfaces of their own, most connections through them; the locals
    kept below the classifier's 64 rules): both blocks' words loaded with
    the connection's fields (kConnEarlyBlocks)."""
    from test_gpu_connect_scale import build, traffic
    rec = Recorder()
    ifs, bind, by_name, pool, spec = build(rec, 13, n_local=6, n_if=20, cfg=3)
    for k, (name, rules, ing, eg) in enumerate(rec.acls):
        if name != "global" and len(rules) >= 64:
            rec.acls[k] = (name, rules[:40], ing, eg)
            by_name[name] = rules[:40]
    big2, _ = random_acl(4242, 3000, 0.0)
    rec.acls.append(("big2", big2, ["bx0", "bx1"], ["bx1", "bx2"]))
    by_name["big2"] = big2
    ifs = ifs + ["bx0", "bx1", "bx2"]
    bind.update({"bx0": ["big2", None], "bx1": ["big2", "big2"], "bx2": [None, "big2"]})
    n = 20000
    tr = traffic(13, n, pool, spec, 4)
    rng = np.random.default_rng(13)
    hot = np.array([0, 1, 2, len(ifs) - 3, len(ifs) - 2, len(ifs) - 1])   # the two large ACLs' interfaces
    si = np.where(rng.random(n) < 0.6, rng.choice(hot, n), rng.integers(0, len(ifs), n))
    di = np.where(rng.random(n) < 0.6, rng.choice(hot, n), rng.integers(0, len(ifs), n))
    verdict, rows = oracle_rows(bind, by_name, ifs, si, di, tr, 4)
    w = {"rec": rec, "ifs": ifs, "bind": bind, "by_name": by_name, "tr": tr, "si": si, "di": di, "verdict": verdict,
         "rows": rows}
    # both large ACLs traced, on rules of their own
    for name in ("global", "big2"):
        first = np.array([bind[ifs[a]][0] == name for a in si])
        assert (first & (rows[:, 0] >= 0) & (rows[:, 0] < len(by_name[name]))).sum() > 300, name
    eng = _engine(debug_conn=1)
    try:
        rec.install(eng)
        capfd.readouterr()
        _check(eng, w, "classifier", True)
        plans = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("connect:") and " trace 1 " in ln]
        assert len(plans) == 1 and " big 2 " in plans[0] and " pre_rules 1 pre_bytes 2" in plans[0], plans
    finally:
        eng.close()


def test_same_interface_reflect():
    """si == di and the first call reflects: testConnection makes no other
    call -- [rule, -1, -1, -1] and ALLOW."""
    w = workload(0, 4, 64)
    rows, v = w["rows"], w["verdict"]
    # (a PERMIT of the first call would go on to the interface's inbound ACL
    # -- the same, non-nil one -- as call 2: only a REFLECT gives this row)
    refl = np.nonzero((w["si"] == w["di"]) & (rows[:, 0] >= 0) & (rows[:, 1:] == -1).all(1) & (v == 2))[0]
    assert refl.size >= 20, refl.size
    eng = _engine()
    try:
        w["rec"].install(eng)
        for device in (False, True):
            gv, gr = _check(eng, w, "auto", device, refl)
            assert (gv == 2).all() and (gr[:, 0] >= 0).all() and (gr[:, 1:] == -1).all()
    finally:
        eng.close()


def test_unknown_and_unbound_interfaces():
    """A device batch's unknown interface id: FAILURE and four -1 there, the
    neighbours unaffected; a host batch with one, and CLS_F_COUNT, are
    CLS_E_INVAL.  Connections between two interfaces without ACLs: ALLOW and
    four -1."""
    import ctypes as C

    from vpp_amd.engine import _ptr
    w = workload(1, 4, 12)
    n = len(w["verdict"])
    bind, ifs = w["bind"], w["ifs"]
    free = np.array([bind[ifs[a]] == [None, None] and bind[ifs[b]] == [None, None] for a, b in zip(w["si"], w["di"])])
    assert free.sum() >= 400
    assert (w["verdict"][free] == 2).all() and (w["rows"][free] == -1).all()
    bad = np.zeros(n, bool)
    bad[np.random.default_rng(1).choice(n, 500, replace=False)] = True
    bad[[0, n - 1]] = True
    eng = _engine()
    try:
        w["rec"].install(eng)
        args = _args(eng, w)
        args[0] = np.where(bad, 1 << 20, args[0]).astype(np.uint32)
        args[1] = np.where(bad & (np.arange(n) % 2 == 0), 0xFFFFFFFF, args[1]).astype(np.uint32)
        dv = [_dev(x) for x in args]
        v, r = eng.connect_rules(*dv)
        v, r = v.cpu().numpy(), r.cpu().numpy()
        assert (v[bad] == 3).all() and (r[bad] == -1).all()
        _same(v[~bad], w["verdict"][~bad], "verdict")
        _same(r[~bad], w["rows"][~bad], "rules")
        assert (v[free & ~bad] == 2).all() and (r[free & ~bad] == -1).all()
        with pytest.raises(_abi.ClsError):
            eng.connect_rules(*args)
        # CLS_F_COUNT: refused (the trace touches no counters)
        good = [np.ascontiguousarray(x) for x in _args(eng, w)]
        pk = _abi.PktSoa(_abi.AF_V4, _ptr(good[2]), _ptr(good[3]), None, None, _ptr(good[5]), _ptr(good[6]),
                         _ptr(good[4]))
        cs = _abi.ConnSoa(pk, _ptr(good[0]), _ptr(good[1]))
        hv, hr = np.zeros(n, np.uint8), np.zeros((n, 4), np.int32)
        fn = _abi.lib().cls_connect_rules
        assert fn(eng.h, C.byref(cs), n, _ptr(hv), _ptr(hr), _abi.F_COUNT, None) == _abi.E_INVAL
        # ... and the verdicts are optional
        assert fn(eng.h, C.byref(cs), n, None, _ptr(hr), 0, None) == 0
        _same(hr, w["rows"], "rules without verdicts")
    finally:
        eng.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_outputs_stay_in_bounds(fam):
    """Device outputs with 64 guard elements past the batch: the guards keep
    their sentinel, and every one of the batch's own entries is written."""
    import torch
    w = workload(0, fam, 64)
    n = len(ODD)
    eng = _engine()
    try:
        w["rec"].install(eng)
        dv = [_dev(x) for x in _args(eng, w, ODD)]
        vbuf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        rbuf = torch.full((n + 16, 4), -2, dtype=torch.int32, device="cuda")
        rbuf[n:] = 0x5A5A5A5A
        v, r = eng.connect_rules(*dv, out=vbuf[:n], rules_out=rbuf[:n])
        assert v.data_ptr() == vbuf.data_ptr() and r.data_ptr() == rbuf.data_ptr()
        torch.cuda.synchronize()
        assert (vbuf[n:] == 0xA5).all() and (rbuf[n:] == 0x5A5A5A5A).all()
        assert not (rbuf[:n] == -2).any() and (vbuf[:n] <= 3).all()
        _same(rbuf[:n].cpu().numpy(), w["rows"][ODD], "rules")
        _same(vbuf[:n].cpu().numpy(), w["verdict"][ODD], "verdict")
        with pytest.raises(_abi.ClsError):
            eng.connect_rules(*dv, rules_out=torch.empty((n, 3), dtype=torch.int32, device="cuda"))
        with pytest.raises(_abi.ClsError):                       # 16-byte alignment
            eng.connect_rules(*dv, rules_out=torch.empty(4 * n + 1, dtype=torch.int32, device="cuda")[1:].view(n, 4))
    finally:
        eng.close()


def test_device_plan_across_batch_kinds_and_a_binding_change():
    """One engine, one device batch: plain, trace, counted, trace, then one
    local ACL put again with other rules, then trace -- the kept plan is per
    batch kind, and nothing stale is read after the change."""
    w = workload(1, 4, 12)
    eng = _engine()
    try:
        w["rec"].install(eng)
        dv = [_dev(x) for x in _args(eng, w, ODD)]

        def trace(want_v, want_r):
            v, r = eng.connect_rules(*dv)
            _same(r.cpu().numpy(), want_r[ODD], "rules")
            _same(v.cpu().numpy(), want_v[ODD], "verdict")

        _same(eng.connect_batch(*dv).cpu().numpy(), w["verdict"][ODD], "plain")
        trace(w["verdict"], w["rows"])
        _same(eng.connect_batch(*dv, count=True).cpu().numpy(), w["verdict"][ODD], "counted")
        trace(w["verdict"], w["rows"])
        trace(w["verdict"], w["rows"])                           # the kept trace plan
        # the local ACL most traced calls are made on, with other rules
        made = [x for row, hit in zip(call_acls(w), w["rows"]) for x, h in zip(row, hit) if h >= 0 and x != "global"]
        name = max(set(made), key=made.count)
        assert made.count(name) > 500
        _, _, ing, eg = next(a for a in w["rec"].acls if a[0] == name)
        rules, _ = random_acl(7777, 150, weird=0.0)
        assert eng.acl_put(name, rules, ing, eg) == 0
        by_name = dict(w["by_name"], **{name: rules})
        v2, r2 = oracle_rows(w["bind"], by_name, w["ifs"], w["si"], w["di"], w["tr"], 4)
        assert (r2 != w["rows"]).any(1).sum() > 100              # the change shows
        trace(v2, r2)
        _same(eng.connect_batch(*dv).cpu().numpy(), v2[ODD], "plain after the change")
        trace(v2, r2)
    finally:
        eng.close()


def test_trace_on_a_callers_stream():
    """A trace batch on a torch stream other than the engine's, read back in
    that stream's order."""
    import torch
    w = workload(1, 16, 12)
    eng = _engine()
    try:
        w["rec"].install(eng)
        dv = [_dev(x) for x in _args(eng, w, ODD)]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        hv = torch.empty(len(ODD), dtype=torch.uint8).pin_memory()
        hr = torch.empty((len(ODD), 4), dtype=torch.int32).pin_memory()
        with torch.cuda.stream(side):
            v, r = eng.connect_rules(*dv, stream=side)
            hv.copy_(v, non_blocking=True)
            hr.copy_(r, non_blocking=True)
        side.synchronize()
        _same(hr.numpy(), w["rows"][ODD], "rules")
        _same(hv.numpy(), w["verdict"][ODD], "verdict")
        # ... and the engine's own stream after it (the scratch is shared)
        v, r = eng.connect_rules(*dv)
        _same(r.cpu().numpy(), w["rows"][ODD], "rules")
    finally:
        eng.close()


def test_renderer_api_names_the_acls_and_rules():
    """ACLEngine.connection_trace on the reference's Connection* KATs
    (acl_renderer_test.go, as test_gpu_parity.py replays them): the actions
    are the expected ones, and the (ACL name, rule) pairs equal
    orc_test_connection_hits on the bound ACLs."""
    import ctypes as C

    import oracle
    from scenario_replay import load_scenarios, replay
    from vpp_amd.engine import ACLEngine, Engine
    seen = {"calls": 0, "traced": 0, "default": 0, "rule": 0}

    def check(engine, calls):
        got = engine.connection_trace(calls)
        assert [g[0] for g in got] == engine.connection_batch(calls)
        for (fn, args), (action, made) in zip(calls, got):
            r = engine.resolve(fn, args)
            if r == 3:
                assert (action, made) == (3, [])
                continue
            sif, sip, dif, dip, proto, sport, dport = r
            acls = [engine.get_inbound_acl(sif), engine.get_outbound_acl(sif), engine.get_inbound_acl(dif),
                    engine.get_outbound_acl(dif)]
            crs = [oracle.rules_to_c(a.rules) if a is not None else None for a in acls]
            refs = [oracle.AclRef(c.ptr(), c.n, 0) if c is not None else oracle.AclRef(None, 0, 1) for c in crs]
            hits = (C.c_int32 * 4)()
            sip, dip = sip or b"", dip or b""
            rc = oracle.lib().orc_test_connection_hits(*[C.byref(x) for x in refs], 1 if sif == dif else 0, sip,
                                                       len(sip), dip, len(dip), proto, sport & 0xFFFF, dport & 0xFFFF,
                                                       hits)
            want = [(a.acl_name, int(h) if h < len(a.rules) else None)
                    for a, h in zip((acls[0], acls[3], acls[2], acls[1]), hits) if h >= 0]
            assert (action, made) == (rc, want), (fn, args, action, made, rc, want)
            seen["calls"] += 1
            seen["traced"] += len(want)
            seen["default"] += sum(1 for _, x in want if x is None)
            seen["rule"] += sum(1 for _, x in want if x is not None)
        return [g[0] for g in got]

    for test in load_scenarios():
        if seen["calls"] >= 48:
            break
        checked, failures = replay(test, lambda contiv: ACLEngine(contiv, Engine()), check_conn=check)
        assert not failures, "\n".join(failures)
    assert seen["calls"] >= 24 and seen["traced"] >= 24 and seen["rule"] >= 8, seen


def _net(b):
    return "-" if not b else "x" + b.hex()


def _write_acls(path, acls):
    with open(path, "w") as f:
        for name, rules, ing, eg in acls:
            f.write("acl %s %d %d %s %d %s\n" % (name, len(rules), len(ing), " ".join(ing), len(eg), " ".join(eg)))
            cr = _abi.CRules(rules)
            for k in range(cr.n):
                r = cr.arr[k]
                f.write("rule %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s %s\n" % (
                    r.flags, r.acl_action, r.tcp_src_lo, r.tcp_src_hi, r.tcp_dst_lo, r.tcp_dst_hi, r.udp_src_lo,
                    r.udp_src_hi, r.udp_dst_lo, r.udp_dst_hi, r.icmp_code_first, r.icmp_code_last,
                    r.icmp_type_first, r.icmp_type_last, _net(r.src_network), _net(r.dst_network)))


@pytest.mark.parametrize("fam", [4, 16])
def test_go_trace_shims(fam, tmp_path):
    """go/shimtest/conntrace (gcc): 20,000 connections through
    clsg_connect_rules_v4 / clsg_connect_rules_v16, as the Go binding's
    ConnectRules calls them."""
    if not os.path.exists(CONNTRACE):
        subprocess.run(["make", "-s", "-C", os.path.dirname(CONNTRACE)], check=True)
    w = workload(0, fam, 12, n_if=LARGE_N_IF)
    _write_acls(tmp_path / "acls.txt", w["rec"].acls)
    (tmp_path / "ifs.txt").write_text("\n".join(w["ifs"]) + "\n")
    tr, m = w["tr"], len(w["verdict"])
    adt = np.uint32 if fam == 4 else np.uint8
    with open(tmp_path / "conn.bin", "wb") as f:
        f.write(np.uint64(m).tobytes())
        for a, dt in ((w["si"], np.uint32), (w["di"], np.uint32), (tr["src"], adt), (tr["dst"], adt),
                      (tr["sport"], np.uint16), (tr["dport"], np.uint16), (tr["proto"], np.uint8)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(
        [os.path.join(ROOT, "vpp_amd")] + [x for x in [os.environ.get("LD_LIBRARY_PATH")] if x]))
    r = subprocess.run([CONNTRACE, str(tmp_path), str(fam)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    _same(np.fromfile(tmp_path / "out_trace_rules.bin", np.int32).reshape(-1, 4), w["rows"], "rules")
    _same(np.fromfile(tmp_path / "out_trace_conn.bin", np.uint8), w["verdict"], "verdict")
