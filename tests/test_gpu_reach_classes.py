"""The reachability classes on the GPU (cls_reach_classes,
Engine.reach_classes, ACLEngine.connection_classes): the endpoints a
reachability matrix cannot tell apart and the quotient matrix between their
classes.

Everything must equal the definition's direct restatement
(reach_classes_cases.classes_ref), bit for bit: on the oracle's matrices of 37
endpoints x 3 probes in the evaluating form with every evaluator (the
evaluated matrix equal to the oracle's), on every synthetic matrix in the
matrix form from host and device memory, with tiles that end inside a row and
inside a probe; the fold's sums and the rounds taken must equal the device-free
twin's (cls_reach_classes_host) bit for bit in both forms, at the full key
width and at 4 bits, which is what catches a lost or doubled atomic; the
device form on a side stream, output subsets, the class_cap retry, the
renderer-level call and the Go shims; every refusal leaves its outputs alone,
and the matrix, diff, port-sweep and hops calls on the same engine are
unaffected."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import reach_classes_cases as cc
from test_gpu_reach import _same, _write_acls
from test_reach_classes_cpu import FIELDS, Host
from vpp_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHCLASSES = os.path.join(ROOT, "go", "shimtest", "reachclasses")
SENTINEL = 0xA5
NAMES = ("classes", "reps", "sizes", "self_", "quotient")
MODES = ("auto", "classifier", "linear")


@pytest.fixture(scope="module")
def engines():
    """Engines by (family with the case installed, or None for an engine
    without ACLs; options), made on first use and shared by the module's
    tests: (engine, the endpoints' interface ids or None)."""
    from vpp_amd.engine import Engine
    made = {}

    def get(fam=None, **opts):
        key = (fam,) + tuple(sorted(opts.items()))
        if key not in made:
            eng = Engine(options=opts or None)
            made[key] = (eng, rc.install(eng, rc.case(fam)) if fam else None)
        return made[key]
    yield get
    for eng, _ in made.values():
        eng.close()


def _args(c, ids, p=None):
    return ids, c["addrs"], c["pr"][:p], c["sp"][:p], c["dp"][:p]


def _fold(eng, m, **kw):
    """The matrix form: nothing but the matrix."""
    return eng.reach_classes(None, None, None, None, None, matrix=m, **kw)


def _host(r):
    """A device-form result as the host form's numpy arrays."""
    kinds = (np.uint32, np.uint32, np.uint32, np.uint8, np.uint8)
    arrs = [x.cpu().numpy().view(k) for x, k in zip(r[:5], kinds)]
    return type(r)(*arrs, r.rounds, None if r.verdict is None else r.verdict.cpu().numpy())


def _check(r, want, m, what):
    """A host-form ReachClasses against classes_ref's tuple and the matrix."""
    from vpp_amd.engine import expand_classes
    for name, g, w in zip(NAMES, r[:5], want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        _same(g, w, "%s: %s" % (what, name))
    assert r.classes[0] == 0 and (np.diff(r.reps.astype(np.int64)) > 0).all(), what
    _same(expand_classes(r.classes, r.self_, r.quotient), m, what + ": expand_classes")
    if r.verdict is not None:
        _same(r.verdict, m, what + ": verdict")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fam, n_classes", [(4, 18), (16, 27)])
def test_oracle_case(fam, n_classes, mode, engines):
    """37 endpoints x 3 probes, evaluated: the classes of the oracle's matrix,
    the evaluated matrix itself, one round."""
    eng, ids = engines(fam)
    c = rc.case(fam)
    want = cc.oracle_ref(fam)
    assert 1 < len(want[1]) < rc.N_EP and len(want[1]) == n_classes
    r = eng.reach_classes(*_args(c, ids), mode=mode, verdict=True)
    assert r.rounds == 1 and r.verdict.shape == (3, 37, 37)
    _check(r, want, c["want"], "family %d, %s" % (fam, mode))
    # without the matrix coming back: a second evaluation behind the fold
    _check(eng.reach_classes(*_args(c, ids), mode=mode), want, c["want"], "family %d, %s, no verdict" % (fam, mode))
    if mode == "auto":
        _check(_fold(eng, np.ascontiguousarray(c["want"])), want, c["want"], "family %d, matrix form" % fam)
        one = eng.reach_classes(*_args(c, ids, 1), verdict=True)
        _check(one, cc.classes_ref(c["want"][:1]), c["want"][:1], "family %d, probe 0 alone" % fam)


@pytest.mark.parametrize("name", cc.NAMES)
def test_synthetic_matrices(name, engines):
    """Every synthetic matrix in the matrix form, from host and from device
    memory, with room for every class and through the class_cap retry."""
    import torch
    eng, _ = engines()
    m = cc.synthetic(name)
    want = cc.synthetic_ref(name)
    r = _fold(eng, m, verdict=True, class_cap=m.shape[1])
    assert r.rounds == 1
    _check(r, want, m, name + ", host")
    _check(_fold(eng, m, class_cap=1), want, m, name + ", host, class_cap 1")
    dm = torch.from_numpy(np.array(m)).cuda()
    r = _fold(eng, dm, device=True, verdict=True)
    assert all(x.is_cuda for x in r[:5]) and r.verdict.is_cuda and r.rounds == 1
    _check(_host(r), want, m, name + ", device")
    _same(dm.cpu().numpy(), m, name + ": the caller's matrix")


def test_tiles(engines):
    """reach_tile 256 (rounded up to 1024): tiles end inside a row and inside
    a probe.  N = 37 evaluated (4,107 cells), N = 130 (50,700 cells) in the
    matrix form from the host and the device."""
    import torch
    for fam in (4, 16):
        c = rc.case(fam)
        small, ids = engines(fam, reach_tile=256)
        assert 37 * 37 % 1024 and 1024 % 37
        for verdict in (True, False):
            r = small.reach_classes(*_args(c, ids), verdict=verdict)
            _check(r, cc.oracle_ref(fam), c["want"], "family %d, reach_tile 256" % fam)
    small, _ = engines(4, reach_tile=256)
    for name in ("planted_130_3_9", "random"):
        m = cc.synthetic(name)
        assert m.shape[1] == 130 and 130 * 130 % 1024 and 1024 % 130
        _check(_fold(small, m, verdict=True), cc.synthetic_ref(name), m, name + ", reach_tile 256, host")
        r = _fold(small, torch.from_numpy(np.array(m)).cuda(), device=True, verdict=True)
        _check(_host(r), cc.synthetic_ref(name), m, name + ", reach_tile 256, device")


class _Raw:
    """cls_reach_classes through ctypes on sentinel-filled host outputs."""

    def __init__(self, eng, c=None, ids=None, m=None):
        from vpp_amd.engine import _ptr
        self.eng, self.ptr = eng, _ptr
        if c is not None:
            self.ids = np.ascontiguousarray(ids, np.uint32)
            self.addrs = np.ascontiguousarray(c["addrs"], np.uint32 if c["fam"] == 4 else np.uint8)
            self.pr, self.sp, self.dp = (np.ascontiguousarray(c[k]) for k in ("pr", "sp", "dp"))
            self.matrix = np.ascontiguousarray(c["want"])
            v16 = c["fam"] == 16
            self.fields = dict(af=_abi.AF_V16 if v16 else _abi.AF_V4, n_endpoints=len(self.ids), if_id=_ptr(self.ids),
                               addr4=None if v16 else _ptr(self.addrs), addr16=_ptr(self.addrs) if v16 else None,
                               n_probes=len(self.pr), proto=_ptr(self.pr), sport=_ptr(self.sp), dport=_ptr(self.dp))
        else:
            self.matrix = np.ascontiguousarray(m)
            self.fields = dict(af=0, n_endpoints=m.shape[1], if_id=None, addr4=None, addr16=None, n_probes=m.shape[0],
                               proto=None, sport=None, dport=None)
        self.h = Host(self.matrix)                       # the outputs and their sentinel
        self.out, self.N, self.P = self.h.out, self.h.N, self.h.P

    def spec(self, **kw):
        f = dict(self.fields, **kw)
        return _abi.ReachSpec(*[f[k] for k, _ in _abi.ReachSpec._fields_])

    def call(self, spec=None, matrix=None, flags=0, out=True, cap=None, **ptrs):
        """ptrs: output name -> replacement (None: leave it out)."""
        o = {k: self.ptr(v) for k, v in self.out.items()}
        o["class_cap"] = self.h.cap if cap is None else cap
        o.update(ptrs)
        st = _abi.ReachClassesOut(*[o[k] for k in FIELDS])
        return _abi.lib().cls_reach_classes(self.eng.h, C.byref(spec or self.spec()), matrix,
                                            C.byref(st) if out else None, flags, None)


@pytest.mark.parametrize("bits", [64, 4])
def test_sums_and_rounds_equal_the_host_twin(bits, engines):
    """sums_out and rounds against cls_reach_classes_host on the same matrix,
    bit for bit: the evaluating form on both oracle cases (untiled and with
    tiles of 1024 cells), the matrix form on synthetic matrices; at the full
    key width and at classes_key_bits = 4, where some take a second round."""
    more = 0
    for fam in (4, 16):
        for opts in ({}, {"reach_tile": 256}):
            eng, ids = engines(fam, **(opts if bits == 64 else dict(opts, classes_key_bits=bits)))
            c = rc.case(fam)
            raw = _Raw(eng, c, ids)
            twin = Host(raw.matrix)
            assert twin.call(key_bits=bits) == 0 and raw.call() == 0
            what = "family %d, %s" % (fam, opts)
            for k in ("sums_out", "rounds", "n_classes", "class_out", "verdict_out"):
                _same(raw.out[k], twin.out[k], "%s: %s" % (what, k))
            for g, w in zip(raw.h.result(), cc.oracle_ref(fam)):
                _same(g, w, what)
    eng, _ = engines(None, **({} if bits == 64 else {"classes_key_bits": bits}))
    for name in ("planted_65_2_7", "planted_64_1_40", "planted_130_3_9", "bytes", "random", "equal", "planted_1_1_1"):
        raw = _Raw(eng, m=cc.synthetic(name))
        twin = Host(raw.matrix)
        assert twin.call(key_bits=bits) == 0 and raw.call(None, raw.ptr(raw.matrix)) == 0
        for k in ("sums_out", "rounds", "n_classes", "class_out"):
            _same(raw.out[k], twin.out[k], "%s: %s" % (name, k))
        for g, w in zip(raw.h.result(), cc.synthetic_ref(name)):
            _same(g, w, name)
        assert raw.out["sums_out"].any() or raw.N == 1
        more += int(raw.out["rounds"][0]) > 1
    # (at 4 bits planted_64_1_40 and random take a second round: ROUNDS of the CPU test)
    assert more == (0 if bits == 64 else 2)


def test_no_convergence_is_reported(engines):
    """classes_key_bits = 0: two classes with equal diagonals never part:
    CLS_E_INVAL with "did not converge", outputs alone; the engine goes on."""
    eng, _ = engines(None, classes_key_bits=0)
    raw = _Raw(eng, m=cc.synthetic("asym_pair"))
    assert raw.call(None, raw.ptr(raw.matrix)) == _abi.E_INVAL and raw.h.untouched()
    assert "did not converge" in _abi.lib().cls_last_error(eng.h).decode()
    raw = _Raw(eng, m=cc.synthetic("diag_pair"))
    assert raw.call(None, raw.ptr(raw.matrix)) == 0 and raw.out["class_out"].tolist() == [0, 0, 0, 1, 0]


@pytest.mark.parametrize("fam", [4, 16])
def test_device_form_and_output_subsets(fam, engines):
    """CLS_F_DEVICE on a side stream; class_out alone, n_classes alone, each
    per-class output alone; the class_cap retry in the evaluating form."""
    import torch
    eng, ids = engines(fam)
    c = rc.case(fam)
    want = cc.oracle_ref(fam)
    side = torch.cuda.Stream()
    for turn in range(2):
        r = eng.reach_classes(*_args(c, ids), device=True, verdict=True, stream=side)
        assert r.classes.is_cuda and r.quotient.is_cuda and r.verdict.is_cuda
        _check(_host(r), want, c["want"], "device, call %d" % turn)       # (complete on return: no synchronize)
    _check(_host(eng.reach_classes(*_args(c, ids), device=True, stream=side)), want, c["want"], "device, no verdict")
    for cap in (1, len(want[1]) - 1, len(want[1])):
        _check(eng.reach_classes(*_args(c, ids), class_cap=cap), want, c["want"], "class_cap %d" % cap)
        _check(_host(eng.reach_classes(*_args(c, ids), class_cap=cap, device=True)), want, c["want"],
               "device, class_cap %d" % cap)
    raw = _Raw(eng, c, ids)
    none = dict.fromkeys(k for k in FIELDS if k != "class_cap")
    n_c = len(want[1])
    subsets = {"class_out": want[0], "n_classes": np.array([n_c], np.uint32), "rep_out": want[1], "size_out": want[2],
               "self_out": want[3].ravel(), "quot_out": want[4].ravel()}
    for name, w in subsets.items():
        raw.h.fill()
        ptrs = dict(none, **{name: raw.ptr(raw.out[name])})
        if name not in ("class_out", "n_classes"):
            ptrs["n_classes"] = raw.ptr(raw.out["n_classes"])
        assert raw.call(cap=n_c, **ptrs) == 0, name
        _same(raw.out[name][:len(w)], w, name + " alone")
        assert raw.h.untouched(*[k for k in raw.out if k not in (name, "n_classes")]), name
    # too small a class_cap: the per-class outputs stay, the classes and the count come
    raw.h.fill()
    assert raw.call(cap=n_c - 1) == 0
    assert raw.h.untouched("rep_out", "size_out", "self_out", "quot_out") and int(raw.out["n_classes"][0]) == n_c
    _same(raw.out["class_out"], want[0], "class_cap too small: classes")
    with pytest.raises(_abi.ClsError):                   # a GPU matrix needs the device form
        _fold(eng, torch.zeros((1, 4, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(_abi.ClsError):
        _fold(eng, np.zeros((1, 4, 5), np.uint8))


def test_refusals_leave_the_outputs_alone(engines):
    """Every CLS_E_INVAL of cls_reach_classes, in both forms, on
    sentinel-filled outputs; the next valid call still matches."""
    import torch
    eng, ids = engines(4)
    c = rc.case(4)
    raw = _Raw(eng, c, ids)
    N, P = raw.N, raw.P
    bad = raw.ids.copy()
    bad[N // 2] = 1 << 20
    mat = raw.ptr(raw.matrix)
    bare = dict(if_id=None, addr4=None, proto=None, sport=None, dport=None)     # what the matrix form may omit
    d = dict(class_out=torch.zeros(N + 1, dtype=torch.int32, device="cuda"),
             rep_out=torch.zeros(N + 1, dtype=torch.int32, device="cuda"),
             size_out=torch.zeros(N + 1, dtype=torch.int32, device="cuda"),
             self_out=torch.zeros(P * N, dtype=torch.uint8, device="cuda"),
             quot_out=torch.zeros(P * N * N, dtype=torch.uint8, device="cuda"),
             verdict_out=torch.zeros(P * N * N + 16, dtype=torch.uint8, device="cuda"))
    dmat = torch.zeros(P * N * N + 16, dtype=torch.uint8, device="cuda")
    ok = {k: t.data_ptr() for k, t in d.items()}
    assert all(p % 16 == 0 for p in ok.values()) and dmat.data_ptr() % 16 == 0
    per_class = dict(rep_out=None, size_out=None, self_out=None, quot_out=None)
    refused = {
        "N = 0": lambda: raw.call(raw.spec(n_endpoints=0)),
        "P = 0": lambda: raw.call(raw.spec(n_probes=0)),
        "bad af": lambda: raw.call(raw.spec(af=6)),
        "NULL if_id": lambda: raw.call(raw.spec(if_id=None)),
        "NULL addr4": lambda: raw.call(raw.spec(addr4=None)),
        "NULL addr16": lambda: raw.call(raw.spec(af=_abi.AF_V16)),
        "NULL proto": lambda: raw.call(raw.spec(proto=None)),
        "NULL sport": lambda: raw.call(raw.spec(sport=None)),
        "NULL dport": lambda: raw.call(raw.spec(dport=None)),
        "unknown interface id": lambda: raw.call(raw.spec(if_id=raw.ptr(bad))),
        "P N^2 > 2^36": lambda: raw.call(raw.spec(n_endpoints=32768, n_probes=65)),
        "N > 32768": lambda: raw.call(raw.spec(n_endpoints=32769, n_probes=1)),
        "out NULL": lambda: raw.call(out=False),
        "neither class_out nor n_classes": lambda: raw.call(class_out=None, n_classes=None),
        "per-class outputs with class_cap 0": lambda: raw.call(cap=0),
        "CLS_F_NO_VERDICT": lambda: raw.call(flags=_abi.F_NO_VERDICT),
        "CLS_F_COUNT": lambda: raw.call(flags=_abi.F_COUNT),
        "matrix: N = 0": lambda: raw.call(raw.spec(n_endpoints=0, **bare), mat),
        "matrix: P = 0": lambda: raw.call(raw.spec(n_probes=0, **bare), mat),
        "matrix: P N^2 > 2^36": lambda: raw.call(raw.spec(n_endpoints=32768, n_probes=65, **bare), mat),
        "matrix: N > 32768": lambda: raw.call(raw.spec(n_endpoints=32769, n_probes=1, **bare), mat),
        "matrix: CLS_F_COUNT": lambda: raw.call(None, mat, flags=_abi.F_COUNT),
        "matrix: CLS_F_CONN_CLS": lambda: raw.call(None, mat, flags=_abi.F_CONN_CLS),
        "matrix: CLS_F_FORCE_LINEAR": lambda: raw.call(None, mat, flags=_abi.F_FORCE_LINEAR),
        "matrix: CLS_F_NO_VERDICT": lambda: raw.call(None, mat, flags=_abi.F_NO_VERDICT),
        "matrix: out NULL": lambda: raw.call(None, mat, out=False),
        "matrix: neither class_out nor n_classes": lambda: raw.call(None, mat, class_out=None, n_classes=None),
        "matrix: per-class outputs with class_cap 0": lambda: raw.call(None, mat, cap=0),
        "misaligned device matrix": lambda: raw.call(None, dmat.data_ptr() + 8, flags=_abi.F_DEVICE, **ok),
    }
    for name, off in (("class_out", 2), ("rep_out", 1), ("size_out", 2), ("verdict_out", 8)):
        refused["misaligned device " + name] = (
            lambda name=name, off=off: raw.call(flags=_abi.F_DEVICE, **dict(ok, **{name: ok[name] + off})))
        refused["matrix: misaligned device " + name] = (
            lambda name=name, off=off: raw.call(None, dmat.data_ptr(), flags=_abi.F_DEVICE,
                                                **dict(ok, **{name: ok[name] + off})))
    for what, f in refused.items():
        raw.h.fill()
        assert f() == _abi.E_INVAL, what
        torch.cuda.synchronize()
        assert raw.h.untouched(), what
        assert not any(bool(t.any()) for t in d.values()), what
    raw.h.fill()
    assert raw.call(raw.spec(n_endpoints=32769, n_probes=1)) == _abi.E_INVAL
    err = _abi.lib().cls_last_error(eng.h).decode()
    assert "32769" in err and "32768" in err, err
    # the matrix form reads nothing of the spec but N and P; class_cap 0 without per-class outputs is fine
    want = cc.oracle_ref(4)
    raw.h.fill()
    assert raw.call(raw.spec(af=0, **bare), mat, cap=0, **per_class) == 0
    _same(raw.out["class_out"], want[0], "a bare spec")
    assert raw.h.untouched("rep_out", "size_out", "self_out", "quot_out") and int(raw.out["rounds"][0]) == 1
    raw.h.fill()
    assert raw.call() == 0
    for g, w in zip(raw.h.result(), want):
        _same(g, w, "raw call after the refusals")
    _same(raw.out["verdict_out"], c["want"], "raw call: verdict")
    # an aligned device call in the matrix form, with HOST count and rounds words
    dmat[:P * N * N] = torch.from_numpy(np.array(raw.matrix).ravel()).cuda()
    raw.h.fill()
    assert raw.call(None, dmat.data_ptr(), flags=_abi.F_DEVICE, sums_out=None, **ok) == 0
    n_c = int(raw.out["n_classes"][0])
    assert n_c == len(want[1]) and int(raw.out["rounds"][0]) == 1
    _same(d["class_out"][:N].cpu().numpy().view(np.uint32), want[0], "device matrix form: classes")
    _same(d["quot_out"][:P * n_c * n_c].cpu().numpy().reshape(P, n_c, n_c), want[4], "device matrix form: quot")
    _same(d["verdict_out"][:P * N * N].cpu().numpy().reshape(P, N, N), c["want"], "device matrix form: verdict copy")


def test_scratch_hygiene(engines):
    """Two classes calls give equal results, and the matrix, the diff, the port
    sweep and the hops on the same engine still match their cases after them."""
    import reach_diff_cases as dc
    import reach_hops_cases as hc
    import reach_ports_cases as pc
    eng, ids = engines(4)
    c = rc.case(4)
    want = cc.oracle_ref(4)
    a = eng.reach_classes(*_args(c, ids), verdict=True)
    m = cc.synthetic("planted_130_3_9")
    _check(_fold(eng, m), cc.synthetic_ref("planted_130_3_9"), m, "a larger matrix in between")
    b = eng.reach_classes(*_args(c, ids), verdict=True)
    for name, x, y in zip(NAMES, a[:5], b[:5]):
        _same(y, x, "second call: " + name)
    v, hist, allow = eng.reach_matrix(*_args(c, ids))
    _same(v, c["want"], "reach_matrix after classes")
    _same(allow, (c["want"] == rc.ALLOW).sum(axis=2), "reach_matrix after classes: allow")
    base = np.array(c["want"])
    base.ravel()[::7] ^= 1
    rec, total, trans, changed = dc.diff_ref(base, c["want"])
    r = eng.reach_diff(*_args(c, ids), base)
    assert r.n_changes == total and r.changes.tobytes() == rec.tobytes()
    _same(r.trans, trans, "reach_diff after classes: trans")
    _check(eng.reach_classes(*_args(c, ids)), want, c["want"], "classes after the diff")
    eps, vb = pc.brute(4, 0)
    ref = pc.ranges_ref(vb)
    p = eng.reach_ports(ids[eps], c["addrs"][eps], 0, pc.SPORT[0])
    assert p.n_ranges == ref[1] and p.ranges.tobytes() == ref[0].tobytes()
    _same(p.runs, ref[2], "reach_ports after classes: runs")
    _check(eng.reach_classes(*_args(c, ids)), want, c["want"], "classes after the sweep")
    _same(eng.reach_hops(*_args(c, ids)).hops, hc.hops_ref(hc.adjacency(c["want"])), "reach_hops after classes")
    _check(eng.reach_classes(*_args(c, ids), verdict=True), want, c["want"], "classes after the hops")


def test_connection_classes_equals_the_matrix_summary():
    """ACLEngine.connection_classes on a replayed renderer scenario plus two
    unregistered pods: the groups, self_ and quotient of classes_ref over
    connection_matrix; the unregistered pods are one group of their own."""
    from scenario_replay import load_scenarios, replay
    from vpp_amd.renderer import api
    from vpp_amd.engine import ACLEngine, Engine
    test = [t for t in load_scenarios() if t["name"] == "TestCombinedRules"][0]
    ghosts = [api.PodID("ghost", "default"), api.PodID("ghost2", "default")]
    seen = []

    def check_gpu(engine, calls):
        probes = sorted({args[2:] for fn, args in calls if fn == "ConnectionPodToPod"})[:2] or [(0, 123, 80)]
        known = sorted(engine.pods, key=lambda p: (p.namespace, p.name))
        for pods in (known, known[:1] + ghosts[:1] + known[1:] + ghosts[1:]):
            m = engine.connection_matrix(pods, probes)
            classes, reps, sizes, self_, quot = cc.classes_ref(m)
            groups, g_self, g_quot = engine.connection_classes(pods, probes)
            assert groups == [[pods[i] for i in np.flatnonzero(classes == k)] for k in range(len(reps))]
            _same(g_self, self_, "self_")
            _same(g_quot, quot, "quotient")
            if len(pods) > len(known):
                assert ghosts in groups
            seen.append(len(groups))
        return engine.connection_batch(calls)

    _, failures = replay(test, lambda contiv: ACLEngine(contiv, Engine()), check_conn=check_gpu)
    assert not failures, "\n".join(failures)
    assert len(seen) >= 2
    eng = ACLEngine(None, Engine())
    try:
        g, s, q = eng.connection_classes([], [(0, 1, 2)])
        assert g == [] and s.shape == (1, 0) and q.shape == (1, 0, 0)
        g, s, q = eng.connection_classes(ghosts, [(0, 1, 2)])
        assert g == [ghosts] and s.shape == (1, 1) and q.shape == (1, 1, 1) and s[0, 0] == q[0, 0, 0]
    finally:
        eng.engine.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_go_shims_reach_classes(fam, tmp_path, engines):
    """go/shimtest/reachclasses (gcc): the oracle case through
    clsg_reach_classes_v4 / clsg_reach_classes_v16, as the Go binding's
    ReachClasses calls them, with room for two classes first; its output files
    equal the Python call's."""
    if not os.path.exists(REACHCLASSES):
        subprocess.run(["make", "-s", "-C", os.path.dirname(REACHCLASSES)], check=True)
    c = rc.case(fam)
    eng, ids = engines(fam)
    want = eng.reach_classes(*_args(c, ids), verdict=True)
    _check(want, cc.oracle_ref(fam), c["want"], "python")
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
    r = subprocess.run([REACHCLASSES, str(tmp_path), str(fam)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    n, p, k = rc.N_EP, len(c["pr"]), len(want.reps)
    assert np.fromfile(tmp_path / "out_classes_n.bin", "<u4").tolist() == [k, 1]
    _same(np.fromfile(tmp_path / "out_classes.bin", "<u4"), want.classes, "classes")
    _same(np.fromfile(tmp_path / "out_classes_rep.bin", "<u4"), want.reps, "reps")
    _same(np.fromfile(tmp_path / "out_classes_size.bin", "<u4"), want.sizes, "sizes")
    _same(np.fromfile(tmp_path / "out_classes_self.bin", np.uint8).reshape(p, k), want.self_, "self")
    _same(np.fromfile(tmp_path / "out_classes_quot.bin", np.uint8).reshape(p, k, k), want.quotient, "quot")
    _same(np.fromfile(tmp_path / "out_classes_verdict.bin", np.uint8).reshape(p, n, n), c["want"], "verdict")
