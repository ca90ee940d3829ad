"""The reachability diff on the GPU (cls_reach_diff, Engine.reach_diff,
ACLEngine.connection_matrix_diff): the changed cells of a matrix against a
baseline.

The new matrix must equal the C oracle's and a fresh cls_reach_matrix; the
records -- in ascending cell index whatever the tiling, the evaluator and the
form -- their total, the transition counts and the changed cells per row must
equal the numpy definition (reach_diff_cases.diff_ref), bit for bit: after a
real ACL change, with nothing changed, on synthetic baselines that put changed
cells on every tile, chunk, wave and group boundary of 4,107 cells, with more
probes than the LDS bins hold, with more chunks than workgroups, under every
cap, in the device form and in place, in every evaluator mode, through the
renderer-level call and the Go shims; and every refusal leaves its outputs
alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import reach_diff_cases as dc
from test_gpu_reach import _same, _sums, _write_acls
from vpp_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHDIFF = os.path.join(ROOT, "go", "shimtest", "reachdiff")
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def engines():
    """Engines with the case installed, by (family, reach_tile or None,
    changed: the ACL change applied), made on first use and shared by the
    module's tests: (engine, the endpoints' interface ids)."""
    from vpp_amd.engine import Engine
    made = {}

    def get(fam, tile=None, changed=False):
        key = (fam, tile, changed)
        if key not in made:
            eng = Engine(options={"reach_tile": tile} if tile else None)
            made[key] = (eng, rc.install(eng, rc.case(fam)))
            if changed:
                dc.apply(eng, rc.case(fam))
        return made[key]
    yield get
    for eng, _ in made.values():
        eng.close()


def _args(c, ids):
    return ids, c["addrs"], c["pr"], c["sp"], c["dp"]


def _check(r, base, new, what, cap=None):
    """A host-form ReachDiff against the numpy definition of base -> new."""
    rec, total, trans, changed = dc.diff_ref(base, new, cap)
    if r.verdicts is not None:
        _same(r.verdicts, new, what + ": verdicts")
    assert r.n_changes == total, (what, r.n_changes, total)
    assert r.changes.dtype == _abi.REACH_CHANGE and len(r.changes) == len(rec), (what, len(r.changes), len(rec))
    for f in ("probe", "src", "dst", "was", "now", "zero"):
        _same(r.changes[f], rec[f], "%s: records' %s" % (what, f))
    if r.trans is not None:
        _same(r.trans, trans, what + ": trans")
    if r.changed is not None:
        _same(r.changed, changed, what + ": changed")
    wh, wa = _sums(new)
    if r.hist is not None:
        _same(r.hist, wh, what + ": hist")
    if r.allow is not None:
        _same(r.allow, wa, what + ": allow")


class _Raw:
    """cls_reach_diff through ctypes on sentinel-filled host outputs."""

    def __init__(self, eng, c, ids, n_rec):
        from vpp_amd.engine import _ptr
        self.eng, self.ptr = eng, _ptr
        self.ids = np.ascontiguousarray(ids, np.uint32)
        fam16 = c["fam"] == 16
        self.addrs = np.ascontiguousarray(c["addrs"], np.uint8 if fam16 else np.uint32)
        self.pr, self.sp, self.dp = (np.ascontiguousarray(c[k]) for k in ("pr", "sp", "dp"))
        self.N, self.P = len(self.ids), len(self.pr)
        N, P = self.N, self.P
        self.fields = dict(af=_abi.AF_V16 if fam16 else _abi.AF_V4, n_endpoints=N, if_id=_ptr(self.ids),
                           addr4=None if fam16 else _ptr(self.addrs), addr16=_ptr(self.addrs) if fam16 else None,
                           n_probes=P, proto=_ptr(self.pr), sport=_ptr(self.sp), dport=_ptr(self.dp))
        self.out = dict(verdict_out=np.zeros((P, N, N), np.uint8), hist_out=np.zeros((P, 4), np.uint64),
                        allow_out=np.zeros((P, N), np.uint32), changes=np.zeros(n_rec, _abi.REACH_CHANGE),
                        n_changes=np.zeros(1, np.uint64), trans_out=np.zeros((P, 4, 4), np.uint64),
                        changed_out=np.zeros((P, N), np.uint32))
        self.fill()

    def fill(self):
        for a in self.out.values():
            a.view(np.uint8).reshape(-1)[:] = SENTINEL

    def untouched(self, *names):
        return all((self.out[k].view(np.uint8) == SENTINEL).all() for k in (names or self.out))

    def spec(self, **kw):
        f = dict(self.fields, **kw)
        return _abi.ReachSpec(*[f[k] for k, _ in _abi.ReachSpec._fields_])

    def outs(self, cap, use, **kw):
        f = {k: self.ptr(self.out[k]) if k in use else None for k in self.out}
        f["cap"] = cap
        f.update(kw)
        return _abi.ReachDiffOut(*[f[k] for k, _ in _abi.ReachDiffOut._fields_])

    def call(self, base, cap, use, flags=0, spec=None, **kw):
        o = self.outs(cap, use, **kw)
        return _abi.lib().cls_reach_diff(self.eng.h, C.byref(spec or self.spec()), self.ptr(base), C.byref(o), flags,
                                         None)


ALL = ("verdict_out", "hist_out", "allow_out", "changes", "n_changes", "trans_out", "changed_out")


@pytest.mark.parametrize("fam", [4, 16])
def test_after_a_real_acl_change(fam):
    """Install, take the base matrix, delete one ACL and re-put another, diff:
    the new matrix is the oracle's after-matrix and a fresh reach_matrix,
    everything else the numpy diff of the two oracle matrices."""
    from vpp_amd.engine import Engine
    c, aft = rc.case(fam), dc.after(fam)
    eng = Engine()
    try:
        ids = rc.install(eng, c)
        base = eng.reach_matrix(*_args(c, ids), hist=False, allow=False)[0]
        _same(base, c["want"], "base")
        dc.apply(eng, c)
        r = eng.reach_diff(*_args(c, ids), base, hist=True, allow=True)
        _check(r, c["want"], aft["want"], "after the change")
        assert r.n_changes == {4: 480, 16: 522}[fam]
        assert not r.changes["zero"].any()                                   # the records' padding
        assert r.changes.tobytes() == dc.diff_ref(c["want"], aft["want"])[0].tobytes()
        _same(r.verdicts, eng.reach_matrix(*_args(c, ids), hist=False, allow=False)[0], "a fresh reach_matrix")
    finally:
        eng.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_nothing_changed(fam, engines):
    """Against the call's own result: no record is written, trans is
    diagonal, changed is zero."""
    c = rc.case(fam)
    eng, ids = engines(fam)
    r = eng.reach_diff(*_args(c, ids), c["want"])
    _check(r, c["want"], c["want"], "unchanged")
    assert r.n_changes == 0 and len(r.changes) == 0 and not r.changed.any()
    assert all((r.trans[p] == np.diag(np.diag(r.trans[p]))).all() for p in range(3))
    raw = _Raw(eng, c, ids, 16)
    assert raw.call(c["want"], 16, ALL) == 0
    assert raw.out["n_changes"][0] == 0 and raw.untouched("changes")
    _same(raw.out["verdict_out"], c["want"], "raw: verdicts")


def _baselines(want):
    """Synthetic baselines of an unchanged matrix: name -> base."""
    flat = want.ravel()
    out = {"every cell": ((want + 1) & 3).astype(np.uint8)}
    edges = [0, 255, 256, 1023, 1024, 4095, 4096, flat.size - 1]

    def flip(cells, to=None):
        b = flat.copy()
        b[cells] = (b[cells] + 1) & 3 if to is None else to
        return b.reshape(want.shape)
    for cell in edges:
        out["cell %d" % cell] = flip([cell])
    out["the edge cells together"] = flip(edges)
    out["the last cell"] = flip([flat.size - 1])
    out["300 cells across 1024"] = flip(np.arange(900, 1200))
    rng = np.random.default_rng(77)
    out["a random half"] = flip(np.flatnonzero(rng.random(flat.size) < 0.5))
    # base bytes above 3: the record carries the byte, trans counts it under & 3
    high = np.array([3, 1022, 1025, 2050, 4104])
    out["bytes above 3"] = flip(high, to=flat[high] | np.array([4, 0x80, 0xFC, 0x40, 0x10], np.uint8))
    return out


@pytest.mark.parametrize("fam", [4, 16])
def test_synthetic_baselines_and_tiling(fam, engines):
    """Unchanged ACLs against baselines with changed cells on the boundaries
    of groups (4), waves (256), tiles (1024) and chunks (4096) and in the
    last, partial group; the default reach_tile (one tile) and 1024 (five
    tiles, the last with 11 cells) give identical results."""
    c = rc.case(fam)
    want = c["want"]
    assert want.size == 4 * 1024 + 11
    (whole, ids), (tiled, ids_t) = engines(fam), engines(fam, 1024)
    for name, base in _baselines(want).items():
        a = whole.reach_diff(*_args(c, ids), base, hist=True, allow=True)
        _check(a, base, want, name)
        b = tiled.reach_diff(*_args(c, ids_t), base, hist=True, allow=True)
        _check(b, base, want, name + ", reach_tile 1024")
        assert a.changes.tobytes() == b.changes.tobytes(), name
    high = whole.reach_diff(*_args(c, ids), _baselines(want)["bytes above 3"])
    assert high.n_changes == 5 and (high.changes["was"] > 3).all() and (high.changes["was"] & 3 ==
                                                                         high.changes["now"]).all()
    assert all((high.trans[p] == np.diag(np.diag(high.trans[p]))).all() for p in range(3))


@pytest.mark.parametrize("fam", [4, 16])
def test_more_probes_than_lds_bins(fam, engines):
    """5 endpoints x 70 probes (the case's three, cyclically): one chunk
    spans more probes than the LDS bins hold, every wave several."""
    c = rc.case(fam)
    at = np.arange(70) % 3
    want = np.ascontiguousarray(c["want"][:3, :5, :5][at])
    rng = np.random.default_rng(78)
    half = want.copy()
    half[rng.random(want.shape) < 0.5] ^= 1
    for tile in (None, 1024):
        eng, ids = engines(fam, tile)
        for name, base in (("a random half", half), ("every cell", ((want + 1) & 3).astype(np.uint8))):
            r = eng.reach_diff(ids[:5], c["addrs"][:5], c["pr"][at], c["sp"][at], c["dp"][at], base, hist=True,
                               allow=True)
            _check(r, base, want, "70 probes, %s, tile %s" % (name, tile))


def test_runs_of_chunks_per_workgroup(engines):
    """The one size at which reach_diff_count takes another path: more chunks
    of 4,096 cells than two workgroups per CU, so that a workgroup takes a
    run of consecutive chunks and carries its LDS bins from one to the next --
    here across probes, each chunk starting in another one (37 endpoints x
    enough probes, the case's three cyclically; about 2.2 M cells on 256
    CUs).  One call; the reference is the case's matrix repeated."""
    import torch
    c = rc.case(4)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    P = ((2 * n_cu + 20) * 4096 + rc.N_EP ** 2 - 1) // rc.N_EP ** 2
    at = np.arange(P) % 3
    want = np.ascontiguousarray(c["want"][at])
    assert want.size > (2 * n_cu + 19) * 4096
    rng = np.random.default_rng(79)
    base = want.copy()
    base[rng.random(want.shape) < 0.01] ^= 2
    base.reshape(-1)[[0, 4095, 4096, 8191, 8192, want.size - 1]] ^= 0x41
    eng, ids = engines(4)
    r = eng.reach_diff(ids, c["addrs"], c["pr"][at], c["sp"][at], c["dp"][at], base, cap=1 << 16, hist=True,
                       allow=True)
    assert 10000 < r.n_changes < 1 << 16
    _check(r, base, want, "%d probes" % P)


@pytest.mark.parametrize("fam", [4, 16])
def test_cap(fam, engines):
    """The real change in five tiles under caps that end in tile 0 (1, 100),
    in tile 1 (200), at the total and past it: n_changes is the full total,
    the first min(total, cap) records are right and in order, the sentinel
    behind them is intact."""
    c, aft = rc.case(fam), dc.after(fam)
    eng, ids = engines(fam, 1024, changed=True)
    rec, total, _, _ = dc.diff_ref(c["want"], aft["want"])
    raw = _Raw(eng, c, ids, total + 8)
    for cap in (1, 100, 200, total, total + 5):
        raw.fill()
        assert raw.call(c["want"], cap, ("changes", "n_changes")) == 0, cap
        k = min(total, cap)
        assert raw.out["n_changes"][0] == total, cap
        assert raw.out["changes"][:k].tobytes() == rec[:k].tobytes(), cap
        assert (raw.out["changes"][k:].view(np.uint8) == SENTINEL).all(), cap
        assert raw.untouched("verdict_out", "hist_out", "allow_out", "trans_out", "changed_out"), cap
        r = eng.reach_diff(*_args(c, ids), c["want"], cap=cap)
        _check(r, c["want"], aft["want"], "cap %d" % cap, cap=cap)


def _dev_records(t, k):
    """The first k rows of a device record tensor as records."""
    return np.ascontiguousarray(t.cpu().numpy()[:k]).view(_abi.REACH_CHANGE).reshape(-1)


@pytest.mark.parametrize("fam", [4, 16])
@pytest.mark.parametrize("tile", [None, 1024])
def test_device_form_and_in_place(fam, tile, engines):
    """Torch tensors on a side stream: outputs allocated by the call and the
    caller's; in place the base tensor becomes the new matrix and a second
    in-place call reports no change; subsets of the outputs."""
    import torch
    from vpp_amd.engine import ReachDiff
    c, aft = rc.case(fam), dc.after(fam)
    eng, ids = engines(fam, tile, changed=True)
    rec, total, trans, changed = dc.diff_ref(c["want"], aft["want"])
    wh, wa = _sums(aft["want"])
    P, N = 3, rc.N_EP
    side = torch.cuda.Stream()
    base = torch.from_numpy(np.array(c["want"])).cuda()
    torch.cuda.synchronize()

    def check(r, what, cap=None):
        side.synchronize()
        k = min(total, total if cap is None else cap)
        if r.verdicts is not None:
            _same(r.verdicts.cpu().numpy(), aft["want"], what + ": verdicts")
        if r.n_changes is not None:
            assert r.n_changes.dtype == torch.int64 and int(r.n_changes[0]) == total, what
        if r.changes is not None:
            assert r.changes.dtype == torch.int32 and r.changes.shape[1] == 4
            assert _dev_records(r.changes, k).tobytes() == rec[:k].tobytes(), what
        if r.trans is not None:
            _same(r.trans.cpu().numpy().astype(np.uint64), trans, what + ": trans")
        if r.changed is not None:
            _same(r.changed.cpu().numpy().astype(np.uint32), changed, what + ": changed")
        if r.hist is not None:
            _same(r.hist.cpu().numpy().astype(np.uint64), wh, what + ": hist")
        if r.allow is not None:
            _same(r.allow.cpu().numpy().astype(np.uint32), wa, what + ": allow")

    r = eng.reach_diff(*_args(c, ids), base, hist=True, allow=True, stream=side)
    assert all(x is not None and x.is_cuda for x in r) and tuple(r.changes.shape) == (P * N * N, 4)
    check(r, "allocated")
    _same(base.cpu().numpy(), c["want"], "the base is left alone")
    # the caller's tensors (overwritten, not added to); the record tensor's 200 rows are the cap
    mine = ReachDiff(torch.full((P, N, N), 7, dtype=torch.uint8, device="cuda"),
                     torch.full((200, 4), -1, dtype=torch.int32, device="cuda"),
                     torch.full((1,), -1, dtype=torch.int64, device="cuda"),
                     torch.full((P, 4, 4), -1, dtype=torch.int64, device="cuda"),
                     torch.full((P, N), -1, dtype=torch.int32, device="cuda"),
                     torch.full((P, 4), -1, dtype=torch.int64, device="cuda"),
                     torch.full((P, N), -1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    r = eng.reach_diff(*_args(c, ids), base, hist=True, allow=True, out=mine, stream=side)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(r, mine))
    check(r, "the caller's tensors", cap=200)
    # subsets of the outputs
    r = eng.reach_diff(*_args(c, ids), base, cap=0, verdicts=False, trans=False, changed=False, stream=side)
    assert [x is None for x in r] == [True, True, False, True, True, True, True]
    check(r, "only n_changes")
    r = eng.reach_diff(*_args(c, ids), base, cap=0, verdicts=False, changed=False, stream=side)
    assert [x is None for x in r] == [True, True, True, False, True, True, True]
    check(r, "only trans")
    r = eng.reach_diff(*_args(c, ids), base, cap=0, verdicts=False, trans=False, stream=side)
    assert [x is None for x in r] == [True, True, True, True, False, True, True]
    check(r, "only changed")
    r = eng.reach_diff(*_args(c, ids), base, verdicts=False, trans=False, changed=False, stream=side)
    assert [x is None for x in r] == [True, False, False, True, True, True, True]
    check(r, "changes without verdicts")
    # in place: behind the call the base is the new matrix
    r = eng.reach_diff(*_args(c, ids), base, inplace=True, stream=side)
    assert r.verdicts.data_ptr() == base.data_ptr()
    check(r, "in place")
    again = eng.reach_diff(*_args(c, ids), base, inplace=True, trans=False, changed=False, stream=side)
    side.synchronize()
    assert int(again.n_changes[0]) == 0
    _same(base.cpu().numpy(), aft["want"], "in place, twice")
    # in place without records or a total: the stores are still made
    base2 = torch.from_numpy(np.array(c["want"])).cuda()
    torch.cuda.synchronize()
    r = eng.reach_diff(*_args(c, ids), base2, cap=0, inplace=True, stream=side)
    check(r, "in place, only trans and changed")
    # the host form in place
    hb = np.array(c["want"])
    r = eng.reach_diff(*_args(c, ids), hb, inplace=True)
    assert r.verdicts is hb
    _check(r, c["want"], aft["want"], "host, in place")


@pytest.mark.parametrize("fam", [4, 16])
def test_modes_and_counters(fam, engines):
    """classifier / linear / auto evaluators give the same diff; with
    count=True the connection counters after one diff are the oracle's
    after-change counters."""
    c, aft = rc.case(fam), dc.after(fam)
    eng, ids = engines(fam, 1024, changed=True)
    got = {}
    for mode in ("classifier", "linear", "auto"):
        got[mode] = eng.reach_diff(*_args(c, ids), c["want"], mode=mode, hist=True, allow=True)
        _check(got[mode], c["want"], aft["want"], mode)
    assert got["classifier"].changes.tobytes() == got["linear"].changes.tobytes() == got["auto"].changes.tobytes()
    for name in aft["by_name"]:
        eng.conn_counters(name, reset=True)
    r = eng.reach_diff(*_args(c, ids), c["want"], count=True)
    _check(r, c["want"], aft["want"], "counting")
    assert sum(int(v.sum()) for v in aft["counts"].values()) > c["want"].size // 4
    for name in aft["by_name"]:
        _same(eng.conn_counters(name, reset=True), aft["counts"][name], "counters of " + name)


def test_refusals(engines):
    """Every CLS_E_INVAL of cls_reach_diff, with an engine: the outputs keep
    their sentinel, and the next valid call still matches."""
    import torch
    c = rc.case(4)
    eng, ids = engines(4)
    want = c["want"]
    raw = _Raw(eng, c, ids, want.size)
    N, P, cells = raw.N, raw.P, want.size
    base = np.array(want)
    lib = _abi.lib()
    bad_ids = raw.ids.copy()
    bad_ids[N // 2] = 1 << 20
    wide = np.zeros(2 * cells, np.uint8)                 # host: verdict_out overlapping base
    wide[:cells] = want.ravel()
    dbase = torch.from_numpy(np.array(want).reshape(-1)).cuda()
    dwide = torch.zeros(2 * cells + 32, dtype=torch.uint8, device="cuda")
    dout = dict(verdict_out=torch.zeros(cells + 16, dtype=torch.uint8, device="cuda"),
                hist_out=torch.zeros(P * 4 + 1, dtype=torch.int64, device="cuda"),
                allow_out=torch.zeros(P * N + 1, dtype=torch.int32, device="cuda"),
                changes=torch.zeros((cells + 1, 4), dtype=torch.int32, device="cuda"),
                n_changes=torch.zeros(2, dtype=torch.int64, device="cuda"),
                trans_out=torch.zeros(P * 16 + 1, dtype=torch.int64, device="cuda"),
                changed_out=torch.zeros(P * N + 1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 0 for t in dout.values()) and dbase.data_ptr() % 16 == 0

    def dev(base_ptr=None, at=None, **off):
        """The device call with some pointers moved by `off` bytes, or `at` an address."""
        f = {k: t.data_ptr() + off.get(k, 0) for k, t in dout.items()}
        f.update(at or {})
        o = _abi.ReachDiffOut(f["verdict_out"], f["hist_out"], f["allow_out"], f["changes"], cells, f["n_changes"],
                              f["trans_out"], f["changed_out"])
        return lib.cls_reach_diff(eng.h, C.byref(raw.spec()), base_ptr or dbase.data_ptr(), C.byref(o), _abi.F_DEVICE,
                                  None)

    assert raw.call(base, cells, ALL) == 0 and dev() == 0
    torch.cuda.synchronize()
    for t in dout.values():
        t.zero_()
    torch.cuda.synchronize()
    diff4 = ("changes", "n_changes", "trans_out", "changed_out")
    refused = {
        "N = 0": lambda: raw.call(base, cells, ALL, spec=raw.spec(n_endpoints=0)),
        "P = 0": lambda: raw.call(base, cells, ALL, spec=raw.spec(n_probes=0)),
        "bad af": lambda: raw.call(base, cells, ALL, spec=raw.spec(af=6)),
        "NULL if_id": lambda: raw.call(base, cells, ALL, spec=raw.spec(if_id=None)),
        "NULL addr4": lambda: raw.call(base, cells, ALL, spec=raw.spec(addr4=None)),
        "NULL proto": lambda: raw.call(base, cells, ALL, spec=raw.spec(proto=None)),
        "unknown interface id": lambda: raw.call(base, cells, ALL, spec=raw.spec(if_id=raw.ptr(bad_ids))),
        "P N^2 > 2^36": lambda: raw.call(base, cells, ALL, spec=raw.spec(n_endpoints=1 << 18, n_probes=2)),
        "NULL spec": lambda: lib.cls_reach_diff(eng.h, None, raw.ptr(base), C.byref(raw.outs(cells, ALL)), 0, None),
        "NULL base": lambda: raw.call(None, cells, ALL),
        "NULL out": lambda: lib.cls_reach_diff(eng.h, C.byref(raw.spec()), raw.ptr(base), None, 0, None),
        "none of the diff outputs": lambda: raw.call(base, 0, ("verdict_out", "hist_out", "allow_out")),
        "changes without n_changes": lambda: raw.call(base, cells, [k for k in ALL if k != "n_changes"]),
        "changes with cap 0": lambda: raw.call(base, 0, ALL),
        "host: verdict_out one byte into base": lambda: raw.call(wide, cells, diff4, verdict_out=raw.ptr(wide) + 1),
        "host: verdict_out ending inside base": lambda: raw.call(wide[cells - 1:], cells, diff4,
                                                                 verdict_out=raw.ptr(wide)),
        "device: verdict_out 16 bytes into base": lambda: dev(base_ptr=dwide.data_ptr(),
                                                              at={"verdict_out": dwide.data_ptr() + 16}),
        "misaligned device base": lambda: dev(base_ptr=dwide.data_ptr() + 4),
        "misaligned device verdict_out": lambda: dev(verdict_out=8),
        "misaligned device hist_out": lambda: dev(hist_out=4),
        "misaligned device allow_out": lambda: dev(allow_out=2),
        "misaligned device changes": lambda: dev(changes=8),
        "misaligned device n_changes": lambda: dev(n_changes=4),
        "misaligned device trans_out": lambda: dev(trans_out=4),
        "misaligned device changed_out": lambda: dev(changed_out=2),
    }
    for what, f in refused.items():
        raw.fill()
        assert f() == _abi.E_INVAL, what
        torch.cuda.synchronize()
        assert raw.untouched(), what
        assert not any(bool(t.any()) for t in dout.values()) and not dwide.any(), what
        assert (wide[:cells] == want.ravel()).all() and not wide[cells:].any(), what
    # adjacent ranges do not overlap; the next valid call still matches
    raw.fill()
    assert raw.call(wide, cells, diff4, verdict_out=raw.ptr(wide) + cells) == 0
    _same(wide[cells:].reshape(want.shape), want, "verdict_out right behind base")
    _check(eng.reach_diff(*_args(c, ids), base), want, want, "after the refusals")


def test_connection_matrix_diff_on_a_replayed_scenario():
    """ACLEngine.connection_matrix_diff on TestCombinedRules (two phases that
    differ in five cells for the chosen probes) over the first phase's pods
    plus an unregistered one: phase k's matrix is the baseline at phase k + 1
    (all CONN_FAILURE before the first); the matrix equals the
    connection_pod_to_pod loop and the change list the numpy diff of the two
    loops, on the GPU engine and against the oracle engine's loops."""
    import oracle
    from scenario_replay import load_scenarios, replay
    from vpp_amd.renderer import api
    from vpp_amd.engine import ACLEngine, Engine
    test = [t for t in load_scenarios() if t["name"] == "TestCombinedRules"][0]
    ghost = api.PodID("ghost", "default")
    seen = {"gpu": [], "oracle": [], "changes": []}
    asked = {}

    def questions(engine, calls):
        if not asked:
            asked["pods"] = sorted(engine.pods, key=lambda p: (p.namespace, p.name)) + [ghost]
            asked["probes"] = sorted({args[2:] for fn, args in calls if fn == "ConnectionPodToPod"})[:2] or \
                [(0, 123, 80)]
        return asked["pods"], asked["probes"]

    def loop(engine, pods, probes):
        return np.array([[[engine.connection_pod_to_pod(s, d, *q) for d in pods] for s in pods] for q in probes],
                        np.uint8)

    def listed(pods, base, new):
        return [(int(p), pods[s], pods[d], int(base[p, s, d]), int(new[p, s, d]))
                for p, s, d in np.argwhere(base != new)]

    def check_gpu(engine, calls):
        pods, probes = questions(engine, calls)
        base = seen["gpu"][-1] if seen["gpu"] else np.full((len(probes), len(pods), len(pods)), 3, np.uint8)
        m, changes = engine.connection_matrix_diff(pods, probes, base)
        assert m.shape == base.shape and m.dtype == np.uint8
        _same(m, loop(engine, pods, probes), "connection_pod_to_pod loop")
        _same(m, engine.connection_matrix(pods, probes), "connection_matrix")
        assert changes == listed(pods, base, m)
        # a baseline that had the unregistered pod reachable: its cells are changes too
        odd = base.copy()
        odd[0, -1, 0], odd[-1, 1, -1] = 2, 0
        m2, changes2 = engine.connection_matrix_diff(pods, probes, odd)
        _same(m2, m, "another baseline, the same matrix")
        assert changes2 == listed(pods, odd, m)
        seen["gpu"].append(m)
        seen["changes"].append(changes)
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
    pods = asked["pods"]
    for k, (g, o) in enumerate(zip(seen["gpu"], seen["oracle"])):
        _same(g, o, "oracle engine, phase %d" % k)
    for k in range(1, len(seen["oracle"])):
        assert seen["changes"][k] == listed(pods, seen["oracle"][k - 1], seen["oracle"][k]), k
    assert any(seen["changes"][k] for k in range(1, len(seen["changes"]))), "no phase pair differs"
    # pods that all fail need no engine call; a baseline of another shape is refused
    eng = ACLEngine(None, Engine())
    try:
        m, changes = eng.connection_matrix_diff([ghost, ghost], [(0, 1, 2)], np.array([[[3, 2], [3, 3]]], np.uint8))
        assert (m == 3).all() and changes == [(0, ghost, ghost, 2, 3)]
        with pytest.raises(_abi.ClsError):
            eng.connection_matrix_diff([ghost], [(0, 1, 2)], np.zeros((1, 2, 2), np.uint8))
    finally:
        eng.engine.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_go_shims_reach_diff(fam, tmp_path, engines):
    """go/shimtest/reachdiff (gcc): the real change through clsg_reach_diff_v4
    / clsg_reach_diff_v16, as the Go binding's ReachDiff calls them; its five
    output files equal the Python call's."""
    if not os.path.exists(REACHDIFF):
        subprocess.run(["make", "-s", "-C", os.path.dirname(REACHDIFF)], check=True)
    c, aft = rc.case(fam), dc.after(fam)
    eng, ids = engines(fam, None, changed=True)
    want = eng.reach_diff(*_args(c, ids), c["want"])
    _check(want, c["want"], aft["want"], "python")
    _write_acls(tmp_path / "acls.txt", aft)
    (tmp_path / "ifs.txt").write_text("\n".join(c["ifs"]) + "\n")
    with open(tmp_path / "reach.bin", "wb") as f:
        f.write(np.array([len(c["at"]), len(c["pr"])], "<u4").tobytes())
        f.write(np.ascontiguousarray(c["at"], "<u4").tobytes())
        f.write(np.ascontiguousarray(c["addrs"], "<u4" if fam == 4 else np.uint8).tobytes())
        f.write(np.ascontiguousarray(c["pr"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(c["sp"], "<u2").tobytes())
        f.write(np.ascontiguousarray(c["dp"], "<u2").tobytes())
    (tmp_path / "base.bin").write_bytes(c["want"].tobytes())
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(
        [os.path.join(ROOT, "vpp_amd")] + [x for x in [os.environ.get("LD_LIBRARY_PATH")] if x]))
    r = subprocess.run([REACHDIFF, str(tmp_path), str(fam)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    P, N = want.verdicts.shape[0], want.verdicts.shape[1]
    _same(np.fromfile(tmp_path / "out_diff_verdict.bin", np.uint8).reshape(P, N, N), want.verdicts, "verdicts")
    assert int(np.fromfile(tmp_path / "out_diff_n.bin", "<u8")[0]) == want.n_changes
    assert (tmp_path / "out_diff_changes.bin").read_bytes() == want.changes.tobytes()
    _same(np.fromfile(tmp_path / "out_diff_trans.bin", "<u8").reshape(P, 4, 4), want.trans, "trans")
    _same(np.fromfile(tmp_path / "out_diff_changed.bin", "<u4").reshape(P, N), want.changed, "changed")
