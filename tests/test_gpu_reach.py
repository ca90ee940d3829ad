"""The reachability matrix on the GPU (cls_reach_matrix, Engine.reach_matrix,
ACLEngine.connection_matrix; reference: ConnectionPodToPod looped over pods
and ports, aclengine_mock.go:243-300).

Every cell (p, s, d) must equal testConnection(if[s], addr[s], if[d], addr[d],
probe p) -- the C oracle's orc_test_connection_hits over the expanded rows,
and the engine's own cls_connect_batch on them -- bit for bit; the histogram
and the allow counts must equal the sums of those cells; tiles that end
inside a row and inside a probe, every evaluator mode, host and device
outputs, counters, refusals, the renderer-level matrix and the Go shims."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reach_cases as rc
from vpp_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHTEST = os.path.join(ROOT, "go", "shimtest", "reachtest")


def _engine(**opts):
    from vpp_amd.engine import Engine
    return Engine(options=opts or None)


def _sums(v):
    """(hist [P, 4], allow [P, N]) of a verdict matrix."""
    hist = np.stack([np.bincount(v[p].ravel(), minlength=4) for p in range(v.shape[0])]).astype(np.uint64)
    return hist, (v == rc.ALLOW).sum(axis=2).astype(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _check_all(res, want, what):
    v, h, a = res
    wh, wa = _sums(want)
    _same(v, want, what + ": verdicts")
    _same(h, wh, what + ": hist")
    _same(a, wa, what + ": allow")


@pytest.mark.parametrize("fam", [4, 16])
def test_matrix_matches_oracle(fam):
    """37 endpoints x 3 probes = 4,107 cells (no multiple of 4 or 64)."""
    c = rc.case(fam)
    want = c["want"]
    assert rc.diverse(want), "the oracle's matrix is degenerate for this seed"
    assert len(set(c["at"].tolist())) < len(c["at"])          # endpoints that share an interface
    eng = _engine()
    try:
        ids = rc.install(eng, c)
        res = eng.reach_matrix(ids, c["addrs"], c["pr"], c["sp"], c["dp"])
        assert res[0].shape == (3, rc.N_EP, rc.N_EP) and res[1].shape == (3, 4) and res[2].shape == (3, rc.N_EP)
        assert res[0].dtype == np.uint8 and res[1].dtype == np.uint64 and res[2].dtype == np.uint32
        _check_all(res, want, "oracle")
        all_ids = np.array([eng.if_id(x) for x in c["ifs"]], np.uint32)
        tr = c["tr"]
        rows = eng.connect_batch(all_ids[c["si"]], all_ids[c["di"]], tr["src"], tr["dst"], tr["proto"], tr["sport"],
                                 tr["dport"])
        _same(res[0].ravel(), rows, "connect_batch on the expanded rows")
    finally:
        eng.close()


def _small(eng, c, ids, n, p):
    """The first n endpoints and p probes of the case."""
    return eng.reach_matrix(ids[:n], c["addrs"][:n], c["pr"][:p], c["sp"][:p], c["dp"][:p])


@pytest.mark.parametrize("fam", [4, 16])
def test_tile_boundaries(fam):
    """reach_tile 256 (the smallest value accepted; rounded up to 1024 like
    every value) and 1024 -- 4,107 cells in five tiles that end inside a row
    and inside a probe, the last one partial -- against the untiled call, and
    the matrices of 1 x 1, 5 x 1 and 64 x 2 (eight whole tiles)."""
    c = rc.case(fam)
    c64 = rc.case(fam, n=64)
    whole = _engine()
    try:
        ids = rc.install(whole, c)
        untiled = whole.reach_matrix(ids, c["addrs"], c["pr"], c["sp"], c["dp"])
        _check_all(untiled, c["want"], "untiled")
        ids64 = rc.install_ids(whole, c64)
        small = {(n, p): _small(whole, c64, ids64, n, p) for n, p in ((1, 1), (5, 1), (64, 2))}
        for (n, p), res in small.items():
            _check_all(res, c64["want"][:p, :n, :n], "untiled %d x %d" % (n, p))
    finally:
        whole.close()
    for tile in (256, 1024):
        eng = _engine(reach_tile=tile)
        try:
            ids = rc.install(eng, c)
            got = eng.reach_matrix(ids, c["addrs"], c["pr"], c["sp"], c["dp"])
            for g, w, what in zip(got, untiled, ("verdicts", "hist", "allow")):
                _same(g, w, "tile %d: %s" % (tile, what))
            ids64 = rc.install_ids(eng, c64)
            for (n, p), w in small.items():
                for g, x, what in zip(_small(eng, c64, ids64, n, p), w, ("verdicts", "hist", "allow")):
                    _same(g, x, "tile %d, %d x %d: %s" % (tile, n, p, what))
        finally:
            eng.close()
    with pytest.raises(_abi.ClsError):
        _engine(reach_tile=255)


@pytest.mark.parametrize("fam", [4, 16])
def test_modes_and_outputs(fam):
    """classifier / linear / auto evaluators; device outputs through torch
    tensors (given and allocated), without verdicts (CLS_F_NO_VERDICT, a NULL
    pointer), hist only and allow only."""
    import torch
    c = rc.case(fam)
    want = c["want"]
    wh, wa = _sums(want)
    args = (c["addrs"], c["pr"], c["sp"], c["dp"])
    eng = _engine()
    try:
        ids = rc.install(eng, c)
        for mode in ("classifier", "linear", "auto"):
            _check_all(eng.reach_matrix(ids, *args, mode=mode), want, mode)
        # host: parts of the outputs
        v, h, a = eng.reach_matrix(ids, *args, verdicts=False)
        assert v is None
        _same(h, wh, "host, no verdicts: hist")
        _same(a, wa, "host, no verdicts: allow")
        v, h, a = eng.reach_matrix(ids, *args, hist=False, allow=False)
        assert h is None and a is None
        _same(v, want, "host, verdicts only")
        # device outputs: allocated, then the caller's (overwritten, not added to)
        dv, dh, da = eng.reach_matrix(ids, *args, out=(None, None, None))
        assert dv.is_cuda and dh.is_cuda and da.is_cuda
        torch.cuda.synchronize()
        _check_all((dv.cpu().numpy(), dh.cpu().numpy().astype(np.uint64), da.cpu().numpy().astype(np.uint32)), want,
                   "device")
        P, N = want.shape[0], want.shape[1]
        mine = (torch.full((P, N, N), 7, dtype=torch.uint8, device="cuda"),
                torch.full((P, 4), 7, dtype=torch.int64, device="cuda"),
                torch.full((P, N), 7, dtype=torch.int32, device="cuda"))
        for mode in ("classifier", "linear"):
            got = eng.reach_matrix(ids, *args, mode=mode, out=mine)
            assert all(g.data_ptr() == m.data_ptr() for g, m in zip(got, mine))
            torch.cuda.synchronize()
            _check_all((mine[0].cpu().numpy(), mine[1].cpu().numpy().astype(np.uint64),
                        mine[2].cpu().numpy().astype(np.uint32)), want, "device, caller's tensors, " + mode)
        side = torch.cuda.Stream()
        for kw, what in ((dict(verdicts=False), "no verdicts"), (dict(verdicts=False, allow=False), "hist only"),
                         (dict(verdicts=False, hist=False), "allow only")):
            v, h, a = eng.reach_matrix(ids, *args, out=(None, None, None), stream=side, **kw)
            side.synchronize()
            assert v is None
            if kw.get("hist", True):
                _same(h.cpu().numpy().astype(np.uint64), wh, "device, %s: hist" % what)
            else:
                assert h is None
            if kw.get("allow", True):
                _same(a.cpu().numpy().astype(np.uint32), wa, "device, %s: allow" % what)
            else:
                assert a is None
        with pytest.raises(_abi.ClsError):
            eng.reach_matrix(ids, *args, out=(torch.empty((P, N, N + 1), dtype=torch.uint8, device="cuda"), None, None))
    finally:
        eng.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_counts_match_oracle(fam):
    """CLS_F_COUNT: the per-(ACL, rule) connection counters after a matrix
    equal the oracle's over its cells; a second call after the reset counts
    the same (outputs overwritten, counters accumulated per call)."""
    c = rc.case(fam)
    eng = _engine(reach_tile=1024)
    try:
        ids = rc.install(eng, c)
        assert sum(int(v.sum()) for v in c["counts"].values()) > c["want"].size // 4
        for turn in range(2):
            res = eng.reach_matrix(ids, c["addrs"], c["pr"], c["sp"], c["dp"], count=True)
            _check_all(res, c["want"], "counting call %d" % turn)
            for name in c["by_name"]:
                _same(eng.conn_counters(name, reset=True), c["counts"][name], "call %d: %s" % (turn, name))
        eng.reach_matrix(ids, c["addrs"], c["pr"], c["sp"], c["dp"], count=True)
        eng.reach_matrix(ids, c["addrs"], c["pr"], c["sp"], c["dp"], count=True)
        eng.reach_matrix(ids, c["addrs"], c["pr"], c["sp"], c["dp"])              # not counted
        for name in c["by_name"]:
            _same(eng.conn_counters(name), 2 * c["counts"][name], "two calls: " + name)
    finally:
        eng.close()


def test_errors():
    """Every CLS_E_INVAL of cls_reach_matrix; nothing is launched by a refused
    call, and the next valid call still matches."""
    import torch
    from vpp_amd.engine import _ptr
    c = rc.case(4)
    eng = _engine()
    try:
        ids = np.ascontiguousarray(rc.install(eng, c), np.uint32)
        a4 = np.ascontiguousarray(c["addrs"], np.uint32)
        a16 = np.zeros((len(ids), 16), np.uint8)
        pr, sp, dp = (np.ascontiguousarray(c[k]) for k in ("pr", "sp", "dp"))
        N, P = len(ids), len(pr)
        v, h, a = np.zeros(P * N * N, np.uint8), np.zeros(P * 4, np.uint64), np.zeros(P * N, np.uint32)
        fn = _abi.lib().cls_reach_matrix

        def spec(**kw):
            f = dict(af=_abi.AF_V4, n_endpoints=N, if_id=_ptr(ids), addr4=_ptr(a4), addr16=None, n_probes=P,
                     proto=_ptr(pr), sport=_ptr(sp), dport=_ptr(dp))
            f.update(kw)
            return _abi.ReachSpec(*[f[k] for k, _ in _abi.ReachSpec._fields_])

        def call(s, vo=v, ho=h, ao=a, flags=0):
            return fn(eng.h, C.byref(s), _ptr(vo), _ptr(ho), _ptr(ao), flags, None)

        assert call(spec()) == 0
        bad_ids = ids.copy()
        bad_ids[N // 2] = 1 << 20
        dv = torch.zeros(P * N * N + 16, dtype=torch.uint8, device="cuda")
        dh = torch.zeros(P * 4 + 1, dtype=torch.int64, device="cuda")
        da = torch.zeros(P * N + 1, dtype=torch.int32, device="cuda")
        assert dv.data_ptr() % 16 == 0
        refused = {
            "N = 0": lambda: call(spec(n_endpoints=0)),
            "P = 0": lambda: call(spec(n_probes=0)),
            "bad af": lambda: call(spec(af=6)),
            "NULL if_id": lambda: call(spec(if_id=None)),
            "NULL addr4": lambda: call(spec(addr4=None)),
            "NULL addr4, af 4 with addr16": lambda: call(spec(addr4=None, addr16=_ptr(a16))),
            "NULL addr16": lambda: call(spec(af=_abi.AF_V16)),
            "NULL proto": lambda: call(spec(proto=None)),
            "NULL sport": lambda: call(spec(sport=None)),
            "NULL dport": lambda: call(spec(dport=None)),
            "no outputs": lambda: call(spec(), None, None, None, _abi.F_NO_VERDICT),
            "NULL verdict_out without CLS_F_NO_VERDICT": lambda: call(spec(), None),
            "P N^2 > 2^36": lambda: call(spec(n_endpoints=1 << 18, n_probes=2)),
            "N > 2^18": lambda: call(spec(n_endpoints=(1 << 18) + 1, n_probes=1)),
            "unknown interface id": lambda: call(spec(if_id=_ptr(bad_ids))),
            "misaligned device verdict_out": lambda: call(spec(), dv[1:], dh, da, _abi.F_DEVICE),
            "misaligned device hist_out": lambda: fn(eng.h, C.byref(spec()), dv.data_ptr(), dh.data_ptr() + 4,
                                                     da.data_ptr(), _abi.F_DEVICE, None),
            "misaligned device allow_out": lambda: fn(eng.h, C.byref(spec()), dv.data_ptr(), dh.data_ptr(),
                                                      da.data_ptr() + 2, _abi.F_DEVICE, None),
            "NULL spec": lambda: fn(eng.h, None, _ptr(v), _ptr(h), _ptr(a), 0, None),
            "NULL engine": lambda: fn(None, C.byref(spec()), _ptr(v), _ptr(h), _ptr(a), 0, None),
        }
        for what, f in refused.items():
            v[:], h[:], a[:] = 9, 9, 9
            assert f() == _abi.E_INVAL, what
            torch.cuda.synchronize()
            assert (v == 9).all() and (h == 9).all() and (a == 9).all(), what       # nothing written
            assert not dv.any() and not dh.any() and not da.any(), what
            # the next valid call still matches
            _check_all(eng.reach_matrix(ids, a4, pr, sp, dp), c["want"], "after: " + what)
        # exactly 2^36 cells is not refused for its size (it is for its unknown interface ids)
        big = np.full(1 << 18, 1 << 20, np.uint32)
        assert call(spec(n_endpoints=1 << 18, n_probes=1, if_id=_ptr(big))) == _abi.E_INVAL
        assert b"unknown interface" in _abi.lib().cls_last_error(eng.h)
    finally:
        eng.close()


def test_connection_matrix_equals_pod_to_pod():
    """ACLEngine.connection_matrix on a replayed renderer scenario
    (TestCombinedRules: three pods, one on another node) plus an unregistered
    pod: cell for cell the nested connection_pod_to_pod loop, on the GPU
    engine and on the oracle's engine."""
    import oracle
    from scenario_replay import load_scenarios, replay
    from vpp_amd.renderer import api
    from vpp_amd.engine import ACLEngine, Engine
    test = [t for t in load_scenarios() if t["name"] == "TestCombinedRules"][0]
    ghost = api.PodID("ghost", "default")
    seen = {"gpu": [], "oracle": []}

    def questions(engine, calls):
        pods = sorted(engine.pods, key=lambda p: (p.namespace, p.name)) + [ghost]
        probes = sorted({args[2:] for fn, args in calls if fn == "ConnectionPodToPod"})[:2]
        return pods, probes or [(0, 123, 80)]

    def loop(engine, pods, probes):
        return np.array([[[engine.connection_pod_to_pod(s, d, *q) for d in pods] for s in pods] for q in probes],
                        np.uint8)

    def check_gpu(engine, calls):
        pods, probes = questions(engine, calls)
        m = engine.connection_matrix(pods, probes)
        assert m.shape == (len(probes), len(pods), len(pods)) and m.dtype == np.uint8
        _same(m, loop(engine, pods, probes), "connection_pod_to_pod loop")
        assert (m[:, -1, :] == 3).all() and (m[:, :, -1] == 3).all()        # the unregistered pod
        assert any(engine.pods[p][1] for p in pods[:-1])                     # one on another node
        seen["gpu"].append(m)
        return engine.connection_batch(calls)

    def check_oracle(engine, calls):
        pods, probes = questions(engine, calls)
        seen["oracle"].append(loop(engine, pods, probes))
        return [getattr(engine, {"ConnectionPodToPod": "connection_pod_to_pod",
                                 "ConnectionPodToInternet": "connection_pod_to_internet",
                                 "ConnectionInternetToPod": "connection_internet_to_pod"}[fn])(*args)
                for fn, args in calls]

    _, failures = replay(test, lambda contiv: ACLEngine(contiv, Engine()), check_conn=check_gpu)
    assert not failures, "\n".join(failures)
    _, failures = replay(test, oracle.OracleACLEngine, check_conn=check_oracle)
    assert not failures, "\n".join(failures)
    assert len(seen["gpu"]) == len(seen["oracle"]) >= 2
    for k, (g, o) in enumerate(zip(seen["gpu"], seen["oracle"])):
        _same(g, o, "oracle engine, phase %d" % k)
    assert len({int(x) for m in seen["gpu"] for x in np.unique(m)}) >= 3
    # an empty pod list, and pods that all fail, need no engine call
    eng = ACLEngine(None, Engine())
    try:
        assert eng.connection_matrix([], [(0, 1, 2)]).shape == (1, 0, 0)
        assert (eng.connection_matrix([ghost, ghost], [(0, 1, 2)]) == 3).all()
    finally:
        eng.engine.close()


def _net(b):
    return "-" if not b else "x" + b.hex()


def _write_acls(path, c):
    """The case's bindings as reachtest reads them: every ACL on the
    interfaces it ends up bound to (an ACL displaced everywhere is left out)."""
    with open(path, "w") as f:
        for name, rules in c["by_name"].items():
            ing = [i for i in c["ifs"] if c["bind"][i][0] == name]
            eg = [i for i in c["ifs"] if c["bind"][i][1] == name]
            if not ing and not eg:
                continue
            f.write("acl %s %d %d %s %d %s\n" % (name, len(rules), len(ing), " ".join(ing), len(eg), " ".join(eg)))
            cr = _abi.CRules(rules)
            for k in range(cr.n):
                r = cr.arr[k]
                f.write("rule %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s %s\n" % (
                    r.flags, r.acl_action, r.tcp_src_lo, r.tcp_src_hi, r.tcp_dst_lo, r.tcp_dst_hi, r.udp_src_lo,
                    r.udp_src_hi, r.udp_dst_lo, r.udp_dst_hi, r.icmp_code_first, r.icmp_code_last,
                    r.icmp_type_first, r.icmp_type_last, _net(r.src_network), _net(r.dst_network)))


@pytest.mark.parametrize("fam", [4, 16])
def test_go_shims_reach(fam, tmp_path):
    """go/shimtest/reachtest (gcc): the case's matrix through
    clsg_reach_matrix_v4 / clsg_reach_matrix_v16, as the Go binding's
    ReachMatrix calls them; its three outputs equal the Python call's."""
    if not os.path.exists(REACHTEST):
        subprocess.run(["make", "-s", "-C", os.path.dirname(REACHTEST)], check=True)
    c = rc.case(fam)
    eng = _engine()
    try:
        ids = rc.install(eng, c)
        want = eng.reach_matrix(ids, c["addrs"], c["pr"], c["sp"], c["dp"])
    finally:
        eng.close()
    _check_all(want, c["want"], "python")
    _write_acls(tmp_path / "acls.txt", c)
    (tmp_path / "ifs.txt").write_text("\n".join(c["ifs"]) + "\n")
    with open(tmp_path / "reach.bin", "wb") as f:
        f.write(np.array([len(c["at"]), len(c["pr"])], "<u4").tobytes())
        f.write(np.ascontiguousarray(c["at"], "<u4").tobytes())
        f.write(np.ascontiguousarray(c["addrs"], "<u4" if fam == 4 else np.uint8).tobytes())
        f.write(np.ascontiguousarray(c["pr"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(c["sp"], "<u2").tobytes())
        f.write(np.ascontiguousarray(c["dp"], "<u2").tobytes())
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(
        [os.path.join(ROOT, "vpp_amd")] + [x for x in [os.environ.get("LD_LIBRARY_PATH")] if x]))
    r = subprocess.run([REACHTEST, str(tmp_path), str(fam)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    P, N = want[0].shape[0], want[0].shape[1]
    _same(np.fromfile(tmp_path / "out_reach_verdict.bin", np.uint8).reshape(P, N, N), want[0], "verdicts")
    _same(np.fromfile(tmp_path / "out_reach_hist.bin", "<u8").reshape(P, 4), want[1], "hist")
    _same(np.fromfile(tmp_path / "out_reach_allow.bin", "<u4").reshape(P, N), want[2], "allow")
