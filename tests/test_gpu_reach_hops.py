"""The hop closure on the GPU (cls_reach_hops, Engine.reach_hops,
ACLEngine.connection_hops): the multi-hop closure and blast radius of the
reachability matrix.

The hop counts must equal the numpy level-synchronous search
(reach_hops_cases.hops_ref) over the union of the probes' ALLOW cells, and
every other output the sums of those hop counts (reach_hops_cases.sums), bit
for bit: on the oracle's matrix of 37 endpoints x 3 probes in the evaluating
form and in the matrix form, on synthetic matrices of graphs no rule table
would produce at sizes around the 64-bit word, from host and device memory,
under every max_hops, with tiles that end inside a row, a probe and a word,
with every evaluator, output subset and block height, in the device form on a
side stream, through the renderer-level call and the Go shims; every refusal
leaves its outputs alone, and the matrix, diff and port-sweep calls on the
same engine are unaffected."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import reach_hops_cases as hc
from test_gpu_reach import _same, _write_acls
from vpp_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHHOPS = os.path.join(ROOT, "go", "shimtest", "reachhops")
SENTINEL = 0xA5
NAMES = ("hops", "reach", "exposed", "levels", "closure")


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
    return eng.reach_hops(None, None, None, None, None, matrix=m, **kw)


def _host(r):
    """A device-form result as the host form's numpy arrays."""
    import torch
    torch.cuda.synchronize()
    kinds = (np.uint8, np.uint32, np.uint32, np.uint64, np.uint64)
    return type(r)(*[None if x is None else x.cpu().numpy().view(k) for x, k in zip(r, kinds)])


def _check(r, hops, what):
    """A host-form ReachHops against the hop counts and their sums; what was
    not asked for is skipped."""
    want = (hops,) + hc.sums(hops)
    for name, g, w in zip(NAMES, r, want):
        if g is not None:
            assert g.dtype == w.dtype, (what, name, g.dtype)
            _same(g, w, "%s: %s" % (what, name))
    n = len(hops)
    if r.closure is not None and n % 64:
        assert not (r.closure[:, -1] >> np.uint64(n % 64)).any(), what + ": closure padding"
    if r.levels is not None:
        assert int(r.levels[0]) == n and int(r.levels.sum()) == n * n, what


@pytest.mark.parametrize("fam, at1, at2, none", [(4, 364, 36, 932), (16, 444, 62, 826)])
def test_oracle_case(fam, at1, at2, none, engines):
    """37 endpoints x 3 probes: the evaluating form against hops_ref of the
    oracle's matrix, the matrix form over that matrix, and one probe alone."""
    eng, ids = engines(fam)
    c = rc.case(fam)
    hops = hc.hops_ref(hc.adjacency(c["want"]))
    lv = hc.sums(hops)[2]
    assert lv[[0, 1, 2, 255]].tolist() == [37, at1, at2, none]          # not degenerate
    r = eng.reach_hops(*_args(c, ids), closure=True)
    assert r.hops.shape == (37, 37) and r.levels.shape == (256,) and r.closure.shape == (37, 1)
    _check(r, hops, "evaluating form")
    _check(_fold(eng, np.ascontiguousarray(c["want"]), closure=True), hops, "matrix form")
    one = eng.reach_hops(*_args(c, ids, 1), closure=True)
    h1 = hc.hops_ref(hc.adjacency(c["want"][:1]))
    _check(one, h1, "probe 0 alone")
    assert (one.hops != r.hops).any()
    if fam == 4:
        assert one.levels[[1, 2, 255]].tolist() == [104, 52, 1176]


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 257])
def test_synthetic_graphs(n, p, engines):
    """Every synthetic graph in the matrix form, from host and from device
    memory: everything equals hops_ref / sums, the closure's padding is zero."""
    import torch
    eng, _ = engines()
    for name in hc.GRAPHS:
        m, a = hc.synthetic(name, n, p)
        hops = hc.synthetic_ref(name, n)[0]
        assert ((hops == 1) == a).all()
        _check(_fold(eng, m, closure=True), hops, "%s %d x %d, host" % (name, n, p))
        dm = torch.from_numpy(np.array(m)).cuda()
        r = _fold(eng, dm, closure=True, out=(None,) * 5)
        assert all(x.is_cuda for x in r)
        _check(_host(r), hops, "%s %d x %d, device" % (name, n, p))


def test_max_hops(engines):
    """A directed path of 300: 254 hops are exact and the 255th is out of
    reach; H = 1 is the adjacency; 3 and 254 equal hops_ref; 255 is refused."""
    from vpp_amd.engine import ClsError
    eng, _ = engines()
    m, a = hc.synthetic("path", 300, 1)
    r = _fold(eng, m, closure=True)
    s, d = np.meshgrid(np.arange(300), np.arange(300), indexing="ij")
    far = d - s
    _same(r.hops, np.where(far == 0, 0, np.where((far > 0) & (far <= 254), far, 255)).astype(np.uint8), "H = 0")
    _check(r, hc.synthetic_ref("path", 300)[0], "H = 0")
    assert int(r.levels[254]) == 46 and int(r.levels[1]) == 299
    r1 = _fold(eng, m, max_hops=1)
    _same(r1.hops == 1, a, "H = 1: the adjacency")
    for H in (1, 3, 254):
        _check(_fold(eng, m, max_hops=H, closure=True), hc.synthetic_ref("path", 300, H)[0], "H = %d" % H)
    before = r.hops.copy()
    with pytest.raises(ClsError):
        _fold(eng, m, max_hops=255)
    with pytest.raises(ClsError):
        _fold(eng, m, max_hops=1 << 20)
    _same(_fold(eng, m).hops, before, "after the refusals")


@pytest.mark.parametrize("tile", [256, 1024])
def test_tiles(tile, engines):
    """reach_tile 256 and 1024 against the untiled call: the oracle cases in
    the evaluating form (4,107 cells: tiles end inside a row and inside a
    probe), a 129 x 3 synthetic matrix from the host and the device (tiles end
    inside a word)."""
    import torch
    for fam in (4, 16):
        c = rc.case(fam)
        (whole, ids), (small, ids_s) = engines(fam), engines(fam, reach_tile=tile)
        a = whole.reach_hops(*_args(c, ids), closure=True)
        b = small.reach_hops(*_args(c, ids_s), closure=True)
        for name, x, y in zip(NAMES, a, b):
            _same(y, x, "family %d, reach_tile %d: %s" % (fam, tile, name))
        _check(b, hc.hops_ref(hc.adjacency(c["want"])), "reach_tile %d" % tile)
    small, _ = engines(4, reach_tile=tile)
    for name in ("random1", "cliques", "complete"):
        m, _ = hc.synthetic(name, 129, 3)
        assert m.size > 40 * 1024 and 1024 % 129
        hops = hc.synthetic_ref(name, 129)[0]
        _check(_fold(small, m, closure=True), hops, "%s, reach_tile %d, host" % (name, tile))
        r = _fold(small, torch.from_numpy(np.array(m)).cuda(), closure=True, out=(None,) * 5)
        _check(_host(r), hops, "%s, reach_tile %d, device" % (name, tile))


@pytest.mark.parametrize("fam", [4, 16])
def test_modes_outputs_and_counts(fam, engines):
    """classifier / linear / auto evaluators; torch outputs, given and
    allocated, on a side stream; each output alone; count=True leaves the
    connection counters of one whole matrix."""
    import torch
    eng, ids = engines(fam)
    c = rc.case(fam)
    hops = hc.hops_ref(hc.adjacency(c["want"]))
    for mode in ("classifier", "linear", "auto"):
        _check(eng.reach_hops(*_args(c, ids), mode=mode, closure=True), hops, mode)
    side = torch.cuda.Stream()
    mine = (torch.full((37, 37), 7, dtype=torch.uint8, device="cuda"), torch.full((37,), 7, dtype=torch.int32, device="cuda"),
            torch.full((37,), 7, dtype=torch.int32, device="cuda"), torch.full((256,), 7, dtype=torch.int64, device="cuda"),
            torch.full((37, 1), 7, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    for turn in range(2):                                # (the caller's accumulators are overwritten, not added to)
        r = eng.reach_hops(*_args(c, ids), closure=True, out=mine, stream=side)
        assert all(g.data_ptr() == m.data_ptr() for g, m in zip(r, mine))
        side.synchronize()
        _check(_host(r), hops, "device, the caller's tensors, call %d" % turn)
    r = eng.reach_hops(*_args(c, ids), closure=True, out=(None,) * 5, stream=side)
    side.synchronize()
    _check(_host(r), hops, "device, allocated")
    for k, name in enumerate(NAMES):
        kw = {x: x == name for x in NAMES}
        r = eng.reach_hops(*_args(c, ids), **kw)
        assert [x is not None for x in r] == [x == name for x in NAMES]
        _check(r, hops, "host, %s alone" % name)
        r = eng.reach_hops(*_args(c, ids), out=(None,) * 5, stream=side, **kw)
        side.synchronize()
        assert [x is not None for x in r] == [x == name for x in NAMES]
        _check(_host(r), hops, "device, %s alone" % name)
    with pytest.raises(_abi.ClsError):
        eng.reach_hops(*_args(c, ids), out=(torch.empty((37, 38), dtype=torch.uint8, device="cuda"),) + (None,) * 4)
    with pytest.raises(_abi.ClsError):                   # a GPU matrix needs the device form
        _fold(eng, torch.zeros((1, 4, 4), dtype=torch.uint8, device="cuda"))
    # counters: the whole matrix is evaluated, once per call
    for name in c["by_name"]:
        eng.conn_counters(name, reset=True)
    _check(eng.reach_hops(*_args(c, ids), count=True), hops, "counting")
    for name in c["by_name"]:
        _same(eng.conn_counters(name, reset=True), c["counts"][name], "counters: " + name)


@pytest.mark.parametrize("rows", [4, 8, 16])
def test_block_heights(rows, engines):
    """hops_rows 4, 8 and 16 source rows per workgroup: the same outputs, with
    sizes that leave the last workgroup partial."""
    eng, _ = engines(None, hops_rows=rows)
    for name, n in (("random1", 129), ("cliques", 65), ("path", 257), ("random2", 3)):
        m, _ = hc.synthetic(name, n, 3)
        _check(_fold(eng, m, closure=True), hc.synthetic_ref(name, n)[0], "%s %d, %d rows" % (name, n, rows))


class _Raw:
    """cls_reach_hops through ctypes on sentinel-filled host outputs."""

    def __init__(self, eng, c, ids):
        from vpp_amd.engine import _ptr
        self.eng, self.ptr = eng, _ptr
        self.ids = np.ascontiguousarray(ids, np.uint32)
        self.addrs = np.ascontiguousarray(c["addrs"], np.uint32)
        self.pr, self.sp, self.dp = (np.ascontiguousarray(c[k]) for k in ("pr", "sp", "dp"))
        self.N, self.P = N, P = len(self.ids), len(self.pr)
        self.matrix = np.ascontiguousarray(c["want"])
        self.fields = dict(af=_abi.AF_V4, n_endpoints=N, if_id=_ptr(self.ids), addr4=_ptr(self.addrs), addr16=None,
                           n_probes=P, proto=_ptr(self.pr), sport=_ptr(self.sp), dport=_ptr(self.dp))
        self.out = dict(hops_out=np.zeros((N, N), np.uint8), reach_out=np.zeros(N, np.uint32),
                        exposed_out=np.zeros(N, np.uint32), level_out=np.zeros(256, np.uint64),
                        closure_out=np.zeros((N, (N + 63) // 64), np.uint64))
        self.fill()

    def fill(self):
        for a in self.out.values():
            a.view(np.uint8).reshape(-1)[:] = SENTINEL

    def untouched(self, *names):
        return all((self.out[k].view(np.uint8) == SENTINEL).all() for k in (names or self.out))

    def spec(self, **kw):
        f = dict(self.fields, **kw)
        return _abi.ReachSpec(*[f[k] for k, _ in _abi.ReachSpec._fields_])

    def call(self, spec=None, matrix=None, max_hops=0, flags=0, out=True, **ptrs):
        """ptrs: output name -> replacement (None: leave it out)."""
        o = {k: self.ptr(v) for k, v in self.out.items()}
        o.update(ptrs)
        st = _abi.ReachHopsOut(*[o[k] for k, _ in _abi.ReachHopsOut._fields_])
        return _abi.lib().cls_reach_hops(self.eng.h, C.byref(spec or self.spec()), matrix, max_hops,
                                         C.byref(st) if out else None, flags, None)


def test_refusals_leave_the_outputs_alone(engines):
    """Every CLS_E_INVAL of cls_reach_hops, in both forms, on sentinel-filled
    outputs; the next valid call still matches."""
    import torch
    eng, ids = engines(4)
    c = rc.case(4)
    raw = _Raw(eng, c, ids)
    N, P = raw.N, raw.P
    bad = raw.ids.copy()
    bad[N // 2] = 1 << 20
    none = dict(hops_out=None, reach_out=None, exposed_out=None, level_out=None, closure_out=None)
    mat = raw.ptr(raw.matrix)
    bare = dict(if_id=None, addr4=None, proto=None, sport=None, dport=None)     # what the matrix form may omit
    d = dict(hops_out=torch.zeros(N * N + 16, dtype=torch.uint8, device="cuda"),
             reach_out=torch.zeros(N + 1, dtype=torch.int32, device="cuda"),
             exposed_out=torch.zeros(N + 1, dtype=torch.int32, device="cuda"),
             level_out=torch.zeros(257, dtype=torch.int64, device="cuda"),
             closure_out=torch.zeros(N + 1, dtype=torch.int64, device="cuda"))
    dmat = torch.zeros(P * N * N + 16, dtype=torch.uint8, device="cuda")
    ok = {k: t.data_ptr() for k, t in d.items()}
    assert all(p % 16 == 0 for p in ok.values()) and dmat.data_ptr() % 16 == 0
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
        "out NULL": lambda: raw.call(out=False),
        "no outputs": lambda: raw.call(**none),
        "CLS_F_NO_VERDICT": lambda: raw.call(flags=_abi.F_NO_VERDICT),
        "max_hops 255": lambda: raw.call(max_hops=255),
        "max_hops 2^31": lambda: raw.call(max_hops=1 << 31),
        "matrix: N = 0": lambda: raw.call(raw.spec(n_endpoints=0, **bare), mat),
        "matrix: P = 0": lambda: raw.call(raw.spec(n_probes=0, **bare), mat),
        "matrix: P N^2 > 2^36": lambda: raw.call(raw.spec(n_endpoints=32768, n_probes=65, **bare), mat),
        "matrix: CLS_F_COUNT": lambda: raw.call(None, mat, flags=_abi.F_COUNT),
        "matrix: CLS_F_CONN_CLS": lambda: raw.call(None, mat, flags=_abi.F_CONN_CLS),
        "matrix: CLS_F_FORCE_LINEAR": lambda: raw.call(None, mat, flags=_abi.F_FORCE_LINEAR),
        "matrix: CLS_F_NO_VERDICT": lambda: raw.call(None, mat, flags=_abi.F_NO_VERDICT),
        "matrix: out NULL": lambda: raw.call(None, mat, out=False),
        "matrix: no outputs": lambda: raw.call(None, mat, **none),
        "matrix: max_hops 255": lambda: raw.call(None, mat, max_hops=255),
        "misaligned device matrix": lambda: raw.call(None, dmat.data_ptr() + 8, flags=_abi.F_DEVICE, **ok),
    }
    for name, off in (("hops_out", 8), ("reach_out", 2), ("exposed_out", 1), ("level_out", 4), ("closure_out", 4)):
        refused["misaligned device " + name] = (
            lambda name=name, off=off: raw.call(flags=_abi.F_DEVICE, **dict(ok, **{name: ok[name] + off})))
        refused["matrix: misaligned device " + name] = (
            lambda name=name, off=off: raw.call(None, dmat.data_ptr(), flags=_abi.F_DEVICE,
                                                **dict(ok, **{name: ok[name] + off})))
    for what, f in refused.items():
        raw.fill()
        assert f() == _abi.E_INVAL, what
        torch.cuda.synchronize()
        assert raw.untouched(), what
        assert not any(bool(t.any()) for t in d.values()), what
    # N > 32,768, with N in the message, in both forms
    for f in (lambda: raw.call(raw.spec(n_endpoints=32769, n_probes=1)),
              lambda: raw.call(raw.spec(n_endpoints=32769, n_probes=1, **bare), mat)):
        raw.fill()
        assert f() == _abi.E_INVAL and raw.untouched()
        err = _abi.lib().cls_last_error(eng.h).decode()
        assert "32769" in err and "32768" in err, err
    # the matrix form reads nothing of the spec but N and P; one output is enough
    hops = hc.hops_ref(hc.adjacency(c["want"]))
    raw.fill()
    assert raw.call(raw.spec(af=0, **bare), mat, **dict(none, reach_out=raw.ptr(raw.out["reach_out"]))) == 0
    _same(raw.out["reach_out"], hc.sums(hops)[0], "reach alone, a bare spec")
    assert raw.untouched("hops_out", "exposed_out", "level_out", "closure_out")
    raw.fill()
    assert raw.call() == 0
    _check(eng.reach_hops(*_args(c, ids), closure=True), hops, "after the refusals")
    for name, w in zip(raw.out, (hops,) + hc.sums(hops)):
        _same(raw.out[name], w, "raw call: " + name)
    # an aligned device call in the matrix form
    dmat[:P * N * N] = torch.from_numpy(np.array(raw.matrix).ravel()).cuda()
    assert raw.call(None, dmat.data_ptr(), flags=_abi.F_DEVICE, **ok) == 0
    torch.cuda.synchronize()
    _same(d["hops_out"][:N * N].cpu().numpy().reshape(N, N), hops, "device matrix form")
    _same(d["level_out"][:256].cpu().numpy().view(np.uint64), hc.sums(hops)[2], "device matrix form: levels")


def test_scratch_hygiene(engines):
    """Two hops calls give equal results, and the matrix, the diff and the
    port sweep on the same engine still match their cases after them."""
    import reach_diff_cases as dc
    import reach_ports_cases as pc
    eng, ids = engines(4)
    c = rc.case(4)
    a = eng.reach_hops(*_args(c, ids), closure=True)
    m, _ = hc.synthetic("complete", 129, 3)
    _check(_fold(eng, m, closure=True), hc.synthetic_ref("complete", 129)[0], "a larger graph in between")
    b = eng.reach_hops(*_args(c, ids), closure=True)
    for name, x, y in zip(NAMES, a, b):
        _same(y, x, "second call: " + name)
    v, hist, allow = eng.reach_matrix(*_args(c, ids))
    _same(v, c["want"], "reach_matrix after hops")
    _same(allow, (c["want"] == rc.ALLOW).sum(axis=2), "reach_matrix after hops: allow")
    base = np.array(c["want"])
    base.ravel()[::7] ^= 1
    rec, total, trans, changed = dc.diff_ref(base, c["want"])
    r = eng.reach_diff(*_args(c, ids), base)
    assert r.n_changes == total and r.changes.tobytes() == rec.tobytes()
    _same(r.trans, trans, "reach_diff after hops: trans")
    _same(r.changed, changed, "reach_diff after hops: changed")
    _check(eng.reach_hops(*_args(c, ids)), a.hops, "hops after the diff")
    eps, vb = pc.brute(4, 0)
    ref = pc.ranges_ref(vb)
    p = eng.reach_ports(ids[eps], c["addrs"][eps], 0, pc.SPORT[0])
    assert p.n_ranges == ref[1] and p.ranges.tobytes() == ref[0].tobytes()
    _same(p.runs, ref[2], "reach_ports after hops: runs")
    _check(eng.reach_hops(*_args(c, ids), closure=True), a.hops, "hops after the sweep")


def test_connection_hops_equals_matrix_and_search():
    """ACLEngine.connection_hops on a replayed renderer scenario plus an
    unregistered pod: hops_ref of the union of connection_matrix's ALLOW
    cells; the unregistered pod's row and column are 255 but for the diagonal."""
    from scenario_replay import load_scenarios, replay
    from vpp_amd.renderer import api
    from vpp_amd.engine import ACLEngine, Engine
    test = [t for t in load_scenarios() if t["name"] == "TestCombinedRules"][0]
    ghost = api.PodID("ghost", "default")
    seen = []

    def check_gpu(engine, calls):
        pods = sorted(engine.pods, key=lambda p: (p.namespace, p.name)) + [ghost]
        probes = sorted({args[2:] for fn, args in calls if fn == "ConnectionPodToPod"})[:2] or [(0, 123, 80)]
        m = engine.connection_matrix(pods, probes)
        n = len(pods)
        for H in (0, 1):
            h = engine.connection_hops(pods, probes, max_hops=H)
            assert h.shape == (n, n) and h.dtype == np.uint8
            _same(h, hc.hops_ref(hc.adjacency(m), H), "max_hops %d" % H)
            assert (h[-1, :-1] == 255).all() and (h[:-1, -1] == 255).all() and h[-1, -1] == 0
        seen.append(engine.connection_hops(pods, probes))
        return engine.connection_batch(calls)

    _, failures = replay(test, lambda contiv: ACLEngine(contiv, Engine()), check_conn=check_gpu)
    assert not failures, "\n".join(failures)
    assert len(seen) >= 2 and any((h == 1).any() for h in seen)
    eng = ACLEngine(None, Engine())
    try:
        assert eng.connection_hops([], [(0, 1, 2)]).shape == (0, 0)
        assert eng.connection_hops([ghost, ghost], [(0, 1, 2)]).tolist() == [[0, 255], [255, 0]]
    finally:
        eng.engine.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_go_shims_reach_hops(fam, tmp_path, engines):
    """go/shimtest/reachhops (gcc): the oracle case through clsg_reach_hops_v4
    / clsg_reach_hops_v16, as the Go binding's ReachHops calls them; its
    output files equal the Python call's."""
    if not os.path.exists(REACHHOPS):
        subprocess.run(["make", "-s", "-C", os.path.dirname(REACHHOPS)], check=True)
    c = rc.case(fam)
    eng, ids = engines(fam)
    want = eng.reach_hops(*_args(c, ids), closure=True)
    _check(want, hc.hops_ref(hc.adjacency(c["want"])), "python")
    want1 = eng.reach_hops(*_args(c, ids), max_hops=1)
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
    r = subprocess.run([REACHHOPS, str(tmp_path), str(fam)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    n = rc.N_EP
    _same(np.fromfile(tmp_path / "out_hops.bin", np.uint8).reshape(n, n), want.hops, "hops")
    _same(np.fromfile(tmp_path / "out_hops1.bin", np.uint8).reshape(n, n), want1.hops, "hops, max_hops 1")
    _same(np.fromfile(tmp_path / "out_hops_reach.bin", "<u4"), want.reach, "reach")
    _same(np.fromfile(tmp_path / "out_hops_exposed.bin", "<u4"), want.exposed, "exposed")
    _same(np.fromfile(tmp_path / "out_hops_levels.bin", "<u8"), want.levels, "levels")
    _same(np.fromfile(tmp_path / "out_hops_closure.bin", "<u8").reshape(n, 1), want.closure, "closure")
