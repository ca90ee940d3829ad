"""The external sweep on the GPU (cls_reach_external, Engine.reach_external,
ACLEngine.connection_external): per-pod remote address ranges over all of
IPv4, to and from the node's output interface.

The ranges -- maximal, in (dir, probe, src, addr_lo) order whatever the class
decomposition, the tiling, the evaluator and the form -- their total, the runs
and ALLOW addresses per line and the histogram per (direction, probe) must
equal the numpy definition (reach_ext_cases.ranges_ref) of the oracle's
verdicts, bit for bit: at the independently restated class starts for all 37
endpoints x 3 probes x both directions, against a brute force over every
address of a /16 window and 65,536 random addresses for six endpoints, on
hand-made configurations at the sizes where the kernels change path (one, two
and five classes, one endpoint, one direction, class starts at 1 and at
0xFFFFFFFF), with tiles of two lines and of one, with dummy classes, under
every cap, in the device form, after an ACL change, against the connection
batch path, through the renderer-level call and the Go shims; and every
refusal leaves its outputs alone."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import reach_diff_cases as dc
import reach_ext_cases as xc
from test_gpu_reach import _same, _write_acls
from vpp_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHEXT = os.path.join(ROOT, "go", "shimtest", "reachext")
SENTINEL = 0xA5
ALL = np.arange(rc.N_EP)
BOTH = ("egress", "ingress")
FIELDS = ("src", "probe", "dir", "action", "addr_lo", "addr_hi")


@pytest.fixture(scope="module")
def engines():
    """Engines with the case installed, by (family, reach_tile or None,
    changed: the ACL change applied), made on first use and shared by the
    module's tests: (engine, the endpoints' interface ids, if0's id)."""
    from vpp_amd.engine import Engine
    made = {}

    def get(fam, tile=None, changed=False):
        key = (fam, tile, changed)
        if key not in made:
            eng = Engine(options={"reach_tile": tile} if tile else None)
            ids = rc.install(eng, rc.case(fam))
            if changed:
                dc.apply(eng, rc.case(fam))
            made[key] = (eng, ids, eng.if_id(xc.EXT_IF))
        return made[key]
    yield get
    for eng, _, _ in made.values():
        eng.close()


@functools.lru_cache(maxsize=None)
def _ref(fam, changed=False):
    """(the class starts restated over every ACL of the case, ranges_ref of
    the oracle's verdicts at them for all 37 endpoints and both directions)."""
    c = dc.after(fam) if changed else rc.case(fam)
    starts = xc.class_starts(list(c["by_name"].values()))
    v = xc.oracle_at(fam, [0, 1], ALL, starts, changed=changed)
    return starts, xc.ranges_ref(v, starts)


def _sweep(eng, ids, ext, c, eps=ALL, dirs=BOTH, **kw):
    return eng.reach_external(ids[eps], c["addrs"][eps], c["pr"], c["sp"], c["dp"], ext, dirs=dirs, **kw)


def _check(r, ref, what):
    """A host-form result against ranges_ref's tuple."""
    rec, total, runs, allow, hist = ref
    assert r["total"] == total, (what, r["total"], total)
    assert r["ranges"].dtype == _abi.ADDR_RANGE and len(r["ranges"]) == len(rec), (what, len(r["ranges"]), len(rec))
    for f in FIELDS:
        _same(r["ranges"][f], rec[f], "%s: ranges' %s" % (what, f))
    _same(r["runs"], runs, what + ": runs")
    _same(r["allow_addrs"], allow, what + ": allow_addrs")
    _same(r["hist"], hist, what + ": hist")
    assert r["allow_addrs"].dtype == np.uint64 and r["hist"].dtype == np.uint64
    assert (r["hist"].sum(axis=2) == 2 ** 32 * runs.shape[2]).all(), what


def _equal(a, b, what):
    """Two host-form results, byte for byte (n_classes aside)."""
    assert a["total"] == b["total"] and a["ranges"].tobytes() == b["ranges"].tobytes(), what
    assert a["runs"].tobytes() == b["runs"].tobytes() and a["allow_addrs"].tobytes() == b["allow_addrs"].tobytes(), what
    assert a["hist"].tobytes() == b["hist"].tobytes(), what


@pytest.mark.parametrize("mode", ["auto", "classifier", "linear"])
@pytest.mark.parametrize("fam", [4, 16])
def test_full_parity(fam, mode, engines):
    """All 37 endpoints x 3 probes x both directions: every output equals the
    numpy definition of the oracle's verdicts at the restated starts; the
    engine's K is that of the bound ACLs, at most the restatement's, and the
    records do not depend on it."""
    eng, ids, ext = engines(fam)
    c = rc.case(fam)
    starts, ref = _ref(fam)
    r = _sweep(eng, ids, ext, c, mode=mode)
    _check(r, ref, "37 endpoints %s" % mode)
    bound = xc.bound_rules(c, ALL)
    assert r["n_classes"] == len(xc.class_starts(bound)) <= len(starts)
    union = np.unique(np.concatenate([eng.addr_classes(x) for x in bound]))
    assert r["n_classes"] == len(union)


@pytest.mark.parametrize("fam", [4, 16])
def test_maximal_ranges_tile_the_space(fam, engines):
    """For every line the ranges tile [0, 0xFFFFFFFF] in order, neighbours
    differ in action and runs is their number."""
    eng, ids, ext = engines(fam)
    c = rc.case(fam)
    r = _sweep(eng, ids, ext, c)
    rec, p, n = r["ranges"], len(c["pr"]), rc.N_EP
    line = xc.line_of(rec, p, n)
    assert (np.diff(line) >= 0).all() and len(np.unique(line)) == 2 * p * n
    first = np.append(True, line[1:] != line[:-1])
    last = np.append(first[1:], True)
    assert (rec["addr_lo"][first] == 0).all() and (rec["addr_hi"][last] == 0xFFFFFFFF).all()
    inner = ~first
    assert (rec["addr_lo"][inner].astype(np.int64) == rec["addr_hi"][:-1][inner[1:]].astype(np.int64) + 1).all()
    assert (rec["action"][inner] != rec["action"][:-1][inner[1:]]).all()
    assert (rec["addr_lo"] <= rec["addr_hi"]).all() and (rec["action"] < 4).all()
    _same(r["runs"].ravel(), np.bincount(line, minlength=2 * p * n), "runs against the records")
    assert r["total"] == len(rec) == r["runs"].sum()


@functools.lru_cache(maxsize=None)
def _six(fam):
    """The aligned /16 window that holds the most class starts of the case's
    bound ACLs, and six endpoints on interfaces that do not bind `global`:
    those with the most ranges that start inside the window in the reference
    (most of the others see one range across it)."""
    c = rc.case(fam)
    starts = xc.class_starts(xc.bound_rules(c, ALL))
    window = int(np.bincount(starts >> 16).argmax())
    assert ((starts >> 16) == window).sum() >= 8
    free = np.array([e for e in range(rc.N_EP) if "global" not in c["bind"][c["ifs"][c["at"][e]]]])
    rec = _ref(fam)[1][0]
    inside = np.bincount(rec["src"][(rec["addr_lo"] >> 16) == window], minlength=rc.N_EP)[free]
    eps = np.sort(free[np.argsort(-inside, kind="stable")[:6]])
    return eps, window


def _lookup_six(r, addrs):
    """lookup of every (dir, probe, endpoint of six) line at every address:
    [2, 3, 6, len(addrs)]."""
    line, a = np.meshgrid(np.arange(2 * 3 * 6), np.asarray(addrs, np.int64), indexing="ij")
    return xc.lookup(r["ranges"], line.ravel(), a.ravel(), p=3, n=6).reshape(2, 3, 6, len(addrs))


@pytest.mark.parametrize("fam", [4, 16])
def test_window_brute_force(fam, engines):
    """Six endpoints: every address of the /16 window with the most class
    starts through the oracle, both directions and all probes, equals the
    ranges looked up there."""
    eng, ids, ext = engines(fam)
    c = rc.case(fam)
    eps, window = _six(fam)
    r = _sweep(eng, ids, ext, c, eps)
    addrs = np.arange(window << 16, (window + 1) << 16)
    want = xc.oracle_at(fam, [0, 1], eps, addrs)
    assert len(np.unique(want)) >= 3
    _same(_lookup_six(r, addrs), want, "window %#x" % window)


@pytest.mark.parametrize("fam", [4, 16])
def test_random_addresses_brute_force(fam, engines):
    """The same six endpoints at 2^16 uniformly random addresses of the whole
    space."""
    eng, ids, ext = engines(fam)
    c = rc.case(fam)
    eps, _ = _six(fam)
    r = _sweep(eng, ids, ext, c, eps)
    addrs = np.random.default_rng(40 + fam).integers(0, 2 ** 32, 1 << 16)
    _same(_lookup_six(r, addrs), xc.oracle_at(fam, [0, 1], eps, addrs), "random addresses")


# ---- hand-made configurations at the sizes where the kernels change path ----

def _net_rules(nets, action=None):
    """TCP, UDP and protocol-47-blind rules over the networks: (src, dst,
    action) each."""
    from vpp_amd import model as M
    out = []
    for k, (src, dst, act) in enumerate(nets):
        out.append(M.l4_rule(act, src, dst, "tcp" if k % 2 == 0 else "udp", 0, 65535, 0, 65535))
        out.append(M.l4_rule(act, src, dst, "udp" if k % 2 == 0 else "tcp", 0, 65535, 0, 65535))
    return out


def _mini_configs():
    from vpp_amd import model as M
    P, D, R = M.PERMIT, M.DENY, M.REFLECT
    top = "255.255.255.255/32"
    cfg = {}
    # ACLs without networks: one class
    cfg["K = 1"] = dict(acls={"a": ([M.l4_rule(P, "", "", "tcp", 0, 65535, 0, 65535)], ["ifa"], ["ifa"]),
                              "x": (_net_rules([("", "", R)]), ["ext"], [])},
                        eps=[("ifa", 0x0A000001), ("ifb", 0x0A000002), ("ifa", 0x0A000003)], K=1)
    cfg["K = 2"] = dict(acls={"a": (_net_rules([("128.0.0.0/1", "", P), ("", "128.0.0.0/1", R)]), ["ifa"], ["ifa"])},
                        eps=[("ifa", 0x0A000001), ("ifb", 0x0A000002), ("ifa", 0xC0000003)], K=2)
    cfg["K = 5"] = dict(acls={"a": (_net_rules([("10.0.0.0/8", "", P), ("", "192.168.0.0/16", R), ("", "10.0.0.0/8", D),
                                                ("", "", P)]), ["ifa"], ["ifb"]),
                              "x": (_net_rules([("", "10.0.0.0/8", R), ("192.168.0.0/16", "", P)]), ["ext"], ["ext"])},
                        eps=[("ifa", 0x0A000001), ("ifb", 0x0A000002), ("ifa", 0xC0A80003), ("ifb", 0x08080808),
                             ("ifc", 0x0A000005)], K=5)
    cfg["N = 1"] = dict(cfg["K = 5"], eps=[("ifb", 0x0A000002)])
    # class starts at 1 (0.0.0.0/32 ends at 0) and at 0xFFFFFFFF
    cfg["starts at 1 and 0xFFFFFFFF"] = dict(
        acls={"a": (_net_rules([("0.0.0.0/32", "", D), ("", "0.0.0.0/32", D), (top, "", D), ("", top, D), ("", "", P)]),
                    ["ifa"], ["ifa"])},
        eps=[("ifa", 0x0A000001), ("ifb", 0x0A000002)], K=3)
    # the remote interface is an endpoint's; an endpoint on an interface without an ACL
    cfg["ext_if is an endpoint's"] = dict(cfg["K = 5"], eps=[("ext", 0x0A000001), ("ifa", 0x0A000002),
                                                            ("ext", 0xC0A80003), ("nowhere", 0x0A000007)])
    return cfg


def _mini_oracle(cfg, fam, dirs, starts):
    """The oracle's verdicts [D, P, N, K] of a hand-made configuration."""
    import oracle
    names = sorted(cfg["acls"])
    ifs = sorted({"ext"} | {e[0] for e in cfg["eps"]} | {i for a in cfg["acls"].values() for i in a[1] + a[2]})
    tabs = [oracle.FastTable(oracle.rules_to_c(cfg["acls"][x][0])) for x in names]
    if_in, if_out = [-1] * len(ifs), [-1] * len(ifs)
    for t, x in enumerate(names):
        for i in cfg["acls"][x][1]:
            if_in[ifs.index(i)] = t
        for i in cfg["acls"][x][2]:
            if_out[ifs.index(i)] = t
    at = np.array([ifs.index(e[0]) for e in cfg["eps"]])
    pod = np.array([e[1] for e in cfg["eps"]], np.int64)
    pr, sp, dp = _MINI_PROBES
    di, pi, si, ki = (x.ravel() for x in np.meshgrid(np.arange(len(dirs)), np.arange(len(pr)), np.arange(len(at)),
                                                     np.arange(len(starts)), indexing="ij"))
    ing = np.asarray(dirs)[di] == 1
    rem, loc = np.asarray(starts, np.int64)[ki], pod[si]
    src, dst = np.where(ing, rem, loc), np.where(ing, loc, rem)
    if fam == 16:
        src, dst = xc.mapped(src), xc.mapped(dst)
    tr = {"src": src, "dst": dst, "proto": pr[pi], "sport": sp[pi], "dport": dp[pi]}
    ext_at = np.full(len(si), ifs.index("ext"))
    v = oracle.connect_fast(tabs, if_in, if_out, np.where(ing, ext_at, at[si]), np.where(ing, at[si], ext_at), tr,
                            af=fam)
    return v.reshape(len(dirs), len(pr), len(at), len(starts))


_MINI_PROBES = (np.array([0, 1, 47], np.uint8), np.array([40000, 53000, 0], np.uint16),
                np.array([80, 53, 0], np.uint16))


@pytest.mark.parametrize("dirs", [BOTH, ("egress",), ("ingress",)])
@pytest.mark.parametrize("what", ["K = 1", "K = 2", "K = 5", "N = 1", "starts at 1 and 0xFFFFFFFF",
                                  "ext_if is an endpoint's"])
@pytest.mark.parametrize("fam", [4, 16])
def test_edges(fam, what, dirs):
    """The smallest shapes at which each kernel path changes: every output
    against the oracle at the restated starts, for both directions and for
    each alone."""
    from vpp_amd.engine import Engine
    cfg = _mini_configs()[what]
    starts = xc.class_starts([a[0] for a in cfg["acls"].values()])
    assert len(starts) == cfg["K"]
    dv = [xc.DIRS[d] for d in dirs]
    ref = xc.ranges_ref(_mini_oracle(cfg, fam, dv, starts), starts, dirs=dv)
    eng = Engine()
    try:
        for name, (rules, ing, eg) in cfg["acls"].items():
            assert eng.acl_put(name, rules, ing, eg) == 0
        ids = np.array([eng.if_id(e[0]) for e in cfg["eps"]], np.uint32)
        addrs = np.array([e[1] for e in cfg["eps"]], np.int64)
        addrs = xc.mapped(addrs) if fam == 16 else addrs.astype(np.uint32)
        r = eng.reach_external(ids, addrs, *_MINI_PROBES, eng.if_id("ext"), dirs=dirs)
    finally:
        eng.close()
    _check(r, ref, what)
    assert r["n_classes"] == len(starts) and len(np.unique(ref[0]["action"])) >= 2
    if what == "K = 1":
        assert r["total"] == r["runs"].size and (r["runs"] == 1).all()
        assert set(np.unique(r["allow_addrs"]).tolist()) <= {0, 2 ** 32}
        assert (r["ranges"]["addr_lo"] == 0).all() and (r["ranges"]["addr_hi"] == 0xFFFFFFFF).all()
    if "0xFFFFFFFF" in what:
        assert (r["ranges"]["addr_lo"] == 0xFFFFFFFF).any() and (r["ranges"]["addr_lo"] == 1).any()


@pytest.mark.parametrize("fam", [4, 16])
def test_tiles_of_two_lines(fam, engines):
    """reach_tile 1024 (two lines per tile, so chunks cross lines and the
    last tile is short) and the default (one tile) give byte-identical
    outputs."""
    c = rc.case(fam)
    (eng, ids, ext), (small, ids_s, ext_s) = engines(fam), engines(fam, 1024)
    a, b = _sweep(eng, ids, ext, c), _sweep(small, ids_s, ext_s, c)
    assert a["n_classes"] == b["n_classes"] and 1024 // a["n_classes"] == 2
    _equal(a, b, "reach_tile 1024 against the default")
    _check(b, _ref(fam)[1], "reach_tile 1024")


def _dummy_rules(m, taken):
    """One rule without networks and m rules on /32 networks no endpoint has,
    which add 2 m classes."""
    from vpp_amd import model as M
    rules = [M.l4_rule(M.DENY, "", "", "tcp", 1, 1, 1, 1)]
    taken, a = set(int(x) for x in taken), (203 << 24) + (113 << 8) + 1
    while len(rules) < m + 1:
        if not {a - 1, a, a + 1, a + 2} & taken:
            net = "%d.%d.%d.%d/32" % (a >> 24, a >> 16 & 255, a >> 8 & 255, a & 255)
            rules.append(M.l4_rule(M.PERMIT, net, net, "tcp", 0, 65535, 0, 65535))
            taken |= {a, a + 1}
        a += 3
    return rules


@functools.lru_cache(maxsize=None)
def _dummy_ref(fam, eps):
    """The oracle at the class starts with an ACL that never matches bound
    outbound to the unbound interface of endpoint 3 (a bound ACL that matches
    nothing denies, where no ACL permits)."""
    c = rc.case(fam)
    free = c["ifs"][c["at"][3]]
    assert c["bind"][free] == [None, None] and 3 in eps
    e = np.array(eps)
    starts = xc.class_starts(xc.bound_rules(c, e))
    v = xc.oracle_at(fam, [0, 1], e, starts, tables=xc.tables_with(fam, _dummy_rules(0, []), free))
    return free, starts, xc.ranges_ref(v, starts)


@pytest.mark.parametrize("n", [37, 5])
@pytest.mark.parametrize("fam", [4, 16])
def test_dummy_classes(fam, n):
    """An extra ACL of m = 0..3 /32 networks that match nothing, on endpoint
    3's interface: K grows by 2 m, so every line's first row moves across
    chunk, wave and group-of-four boundaries; merging removes the dummy
    boundaries, so all but n_classes is identical across m and equals the
    reference."""
    from vpp_amd.engine import Engine
    c = rc.case(fam)
    eps = tuple(range(37)) if n == 37 else (3,) + tuple(int(x) for x in _six(fam)[0] if x != 3)[:4]
    free, starts, ref = _dummy_ref(fam, eps)
    e = np.array(eps)
    eng = Engine()
    try:
        ids = rc.install(eng, c)
        ext = eng.if_id(xc.EXT_IF)
        first = None
        for m in range(4):
            assert eng.acl_put("dummy", _dummy_rules(m, starts), [], [free]) == 0
            r = _sweep(eng, ids, ext, c, e)
            _check(r, ref, "m = %d" % m)
            assert r["n_classes"] == len(starts) + 2 * m
            first = first or r
            _equal(r, first, "m = %d against m = 0" % m)
    finally:
        eng.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_more_classes_than_a_tile(fam):
    """A dummy ACL of 700 /32 networks: K > reach_tile = 1024, a tile is one
    line's K rows.  Identical to the default tile, and to the reference."""
    from vpp_amd.engine import Engine
    c = rc.case(fam)
    free, starts, ref = _dummy_ref(fam, tuple(range(37)))
    got = []
    for tile in (1024, None):
        eng = Engine(options={"reach_tile": tile} if tile else None)
        try:
            ids = rc.install(eng, c)
            assert eng.acl_put("dummy", _dummy_rules(700, starts), [], [free]) == 0
            got.append(_sweep(eng, ids, eng.if_id(xc.EXT_IF), c))
            assert got[-1]["n_classes"] == len(starts) + 1400 > 1024
            _check(got[-1], ref, "K > tile, reach_tile %s" % tile)
        finally:
            eng.close()
    _equal(got[0], got[1], "K > tile against one tile")


class _Raw:
    """cls_reach_external through ctypes on sentinel-filled host outputs."""

    def __init__(self, eng, c, ids, ext, eps, n_rec, nd=2):
        from vpp_amd.engine import _ptr
        self.eng, self.ptr, self.ext = eng, _ptr, ext
        self.ids = np.ascontiguousarray(ids[eps], np.uint32)
        fam16 = c["fam"] == 16
        self.addrs = np.ascontiguousarray(c["addrs"][eps], np.uint8 if fam16 else np.uint32)
        self.pr, self.sp, self.dp = (np.ascontiguousarray(c[k]) for k in ("pr", "sp", "dp"))
        self.N, self.P = N, P = len(self.ids), len(self.pr)
        self.fields = dict(af=_abi.AF_V16 if fam16 else _abi.AF_V4, n_endpoints=N, if_id=_ptr(self.ids),
                           addr4=None if fam16 else _ptr(self.addrs), addr16=_ptr(self.addrs) if fam16 else None,
                           n_probes=P, proto=_ptr(self.pr), sport=_ptr(self.sp), dport=_ptr(self.dp))
        self.out = dict(ranges=np.zeros(n_rec, _abi.ADDR_RANGE), n_ranges=np.zeros(1, np.uint64),
                        runs_out=np.zeros((nd, P, N), np.uint32), allow_addrs_out=np.zeros((nd, P, N), np.uint64),
                        hist_out=np.zeros((nd, P, 4), np.uint64), n_classes=np.zeros(1, np.uint32))
        self.fill()

    def fill(self):
        for a in self.out.values():
            a.view(np.uint8).reshape(-1)[:] = SENTINEL

    def untouched(self, *names):
        return all((self.out[k].view(np.uint8) == SENTINEL).all() for k in (names or self.out))

    def spec(self, **kw):
        f = dict(self.fields, **kw)
        return _abi.ReachSpec(*[f[k] for k, _ in _abi.ReachSpec._fields_])

    def call(self, spec=None, cap=None, flags=0, ext=None, dirs=3, out=True, **ptrs):
        """ptrs: output name -> replacement (None: leave it out); out False:
        a NULL cls_reach_ext_out."""
        o = {k: self.ptr(v) for k, v in self.out.items()}
        o.update(ptrs)
        cap = len(self.out["ranges"]) if cap is None else cap
        st = _abi.ReachExtOut(o["ranges"], cap, o["n_ranges"], o["runs_out"], o["allow_addrs_out"], o["hist_out"],
                              o["n_classes"])
        return _abi.lib().cls_reach_external(self.eng.h, C.byref(spec or self.spec()),
                                             self.ext if ext is None else ext, dirs, C.byref(st) if out else None,
                                             flags, None)


@pytest.mark.parametrize("fam", [4, 16])
def test_cap(fam, engines):
    """cap 1, total - 1, total and total + 7 on tiles of a few lines: the
    first min(total, cap) records, the sentinels behind them untouched, the
    total and the sums unchanged."""
    small, ids, ext = engines(fam, 2048)
    c = rc.case(fam)
    rec, total, runs, allow, hist = _ref(fam)[1]
    raw = _Raw(small, c, ids, ext, ALL, total + 7)
    for cap in (1, total - 1, total, total + 7):
        raw.fill()
        assert raw.call(cap=cap) == 0, cap
        n = min(cap, total)
        assert int(raw.out["n_ranges"][0]) == total, cap
        assert raw.out["ranges"][:n].tobytes() == rec[:n].tobytes(), cap
        assert (raw.out["ranges"][n:].view(np.uint8) == SENTINEL).all(), cap
        _same(raw.out["runs_out"], runs, "cap %d: runs" % cap)
        _same(raw.out["allow_addrs_out"], allow, "cap %d: allow_addrs" % cap)
        _same(raw.out["hist_out"], hist, "cap %d: hist" % cap)
        assert int(raw.out["n_classes"][0]) == len(xc.class_starts(xc.bound_rules(c, ALL)))
    # the Python call: cap cuts the records, cap 0 asks for none
    r = _sweep(small, ids, ext, c, cap=total // 2)
    assert r["total"] == total and r["ranges"].tobytes() == rec[:total // 2].tobytes()
    r = _sweep(small, ids, ext, c, cap=0)
    assert r["ranges"] is None and r["total"] == total


@pytest.mark.parametrize("fam", [4, 16])
def test_device_form(fam, engines):
    """torch outputs on a side stream equal the host form; n_classes is set on
    return; records past the total stay; each misaligned pointer is refused."""
    import torch
    eng, ids, ext = engines(fam, 2048)
    c = rc.case(fam)
    host = _sweep(eng, ids, ext, c)
    cap = host["total"] + 5
    side = torch.cuda.Stream()
    rg = torch.full((cap, 4), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r = _sweep(eng, ids, ext, c, out=(rg, None, None, None, None), stream=side)
    assert r["n_classes"] == host["n_classes"] and r["ranges"] is rg
    side.synchronize()
    assert int(r["total"].item()) == host["total"]
    got = rg.cpu().numpy()
    assert got[:host["total"]].tobytes() == host["ranges"].tobytes()
    assert (got[host["total"]:] == -1).all()
    _same(r["runs"].cpu().numpy().view(np.uint32), host["runs"], "device runs")
    _same(r["allow_addrs"].cpu().numpy().view(np.uint64), host["allow_addrs"], "device allow_addrs")
    _same(r["hist"].cpu().numpy().view(np.uint64), host["hist"], "device hist")
    # a device cap below the total
    few = torch.full((7, 4), -1, dtype=torch.int32, device="cuda")
    r2 = _sweep(eng, ids, ext, c, out=(few, None, None, None, None))
    torch.cuda.synchronize()
    assert int(r2["total"].item()) == host["total"] and few.cpu().numpy().tobytes() == host["ranges"][:7].tobytes()
    # misaligned device pointers
    raw = _Raw(eng, c, ids, ext, ALL, 1)
    lines = 2 * raw.P * raw.N
    d = dict(ranges=torch.zeros(16 * cap + 16, dtype=torch.uint8, device="cuda"),
             n_ranges=torch.zeros(2, dtype=torch.int64, device="cuda"),
             runs_out=torch.zeros(lines + 1, dtype=torch.int32, device="cuda"),
             allow_addrs_out=torch.zeros(lines + 1, dtype=torch.int64, device="cuda"),
             hist_out=torch.zeros(2 * raw.P * 4 + 1, dtype=torch.int64, device="cuda"))
    ok = {k: t.data_ptr() for k, t in d.items()}
    for name, off in (("ranges", 8), ("n_ranges", 4), ("runs_out", 2), ("allow_addrs_out", 4), ("hist_out", 4)):
        raw.fill()
        assert raw.call(cap=cap, flags=_abi.F_DEVICE, **dict(ok, **{name: ok[name] + off})) == _abi.E_INVAL, name
        torch.cuda.synchronize()
        assert raw.untouched("n_classes") and not any(bool(t.any()) for t in d.values()), name
    assert raw.call(cap=cap, flags=_abi.F_DEVICE, **ok) == 0
    torch.cuda.synchronize()
    assert int(d["n_ranges"][0].item()) == host["total"] and int(raw.out["n_classes"][0]) == host["n_classes"]
    assert d["ranges"][:16 * host["total"]].cpu().numpy().tobytes() == host["ranges"].tobytes()


def test_refusals_leave_the_outputs_alone(engines):
    """Every CLS_E_INVAL of cls_reach_external, on sentinel-filled outputs;
    the next valid call still matches."""
    eng, ids, ext = engines(4)
    c = rc.case(4)
    ref = _ref(4)[1]
    raw = _Raw(eng, c, ids, ext, ALL, ref[1])
    bad = raw.ids.copy()
    bad[3] = 1 << 20
    many = 70000
    none = dict(ranges=None, n_ranges=None, runs_out=None, allow_addrs_out=None, hist_out=None)
    refused = {
        "n_probes 0": lambda: raw.call(raw.spec(n_probes=0)),
        "N = 0": lambda: raw.call(raw.spec(n_endpoints=0)),
        "bad af": lambda: raw.call(raw.spec(af=6)),
        "NULL if_id": lambda: raw.call(raw.spec(if_id=None)),
        "NULL addr4": lambda: raw.call(raw.spec(addr4=None)),
        "NULL proto": lambda: raw.call(raw.spec(proto=None)),
        "NULL sport": lambda: raw.call(raw.spec(sport=None)),
        "NULL dport": lambda: raw.call(raw.spec(dport=None)),
        "dirs 0": lambda: raw.call(dirs=0),
        "dirs 4": lambda: raw.call(dirs=4),
        "dirs 7": lambda: raw.call(dirs=7),
        "unknown ext_if": lambda: raw.call(ext=1 << 20),
        "CLS_F_COUNT": lambda: raw.call(flags=_abi.F_COUNT),
        "CLS_F_NO_VERDICT": lambda: raw.call(flags=_abi.F_NO_VERDICT),
        "unknown interface id": lambda: raw.call(raw.spec(if_id=raw.ptr(bad))),
        "out NULL": lambda: raw.call(out=False),
        "out NULL, device": lambda: raw.call(out=False, flags=_abi.F_DEVICE),
        "no outputs": lambda: raw.call(**none),
        "ranges without n_ranges": lambda: raw.call(n_ranges=None),
        "cap 0": lambda: raw.call(cap=0),
        "N > 2^18": lambda: raw.call(raw.spec(n_endpoints=(1 << 18) + 1)),
        "more than 65536 probes": lambda: raw.call(raw.spec(n_endpoints=1, n_probes=many,
                                                           proto=raw.ptr(np.zeros(many, np.uint8)),
                                                           sport=raw.ptr(np.zeros(many, np.uint16)),
                                                           dport=raw.ptr(np.zeros(many, np.uint16)))),
    }
    for what, f in refused.items():
        raw.fill()
        assert f() == _abi.E_INVAL, what
        assert raw.untouched(), what
    _check(_sweep(eng, ids, ext, c), ref, "after the refusals")
    # one output alone is enough
    raw.fill()
    assert raw.call(**dict(none, hist_out=raw.ptr(raw.out["hist_out"]))) == 0
    _same(raw.out["hist_out"], ref[4], "hist alone")
    assert raw.untouched("ranges", "n_ranges", "runs_out", "allow_addrs_out")


def test_refusal_above_2_36_rows():
    """D P N K > 2^36 within what cls_reach_matrix takes of the spec (P N^2 <=
    2^36): 2 directions x 65,536 probes x 1,024 endpoints = 2^27 lines over an
    ACL of 300 /32 networks (K = 601 > 2^9); K and N are in cls_last_error.
    """
    from vpp_amd.engine import Engine, _ptr
    eng = Engine()
    try:
        assert eng.acl_put("nets", _dummy_rules(300, []), ["ifa"], []) == 0
        n, p = 1024, 65536
        ids, addrs = np.full(n, eng.if_id("ifa"), np.uint32), np.zeros(n, np.uint32)
        pr, sp, dp = np.zeros(p, np.uint8), np.zeros(p, np.uint16), np.zeros(p, np.uint16)
        spec = _abi.ReachSpec(_abi.AF_V4, n, _ptr(ids), _ptr(addrs), None, p, _ptr(pr), _ptr(sp), _ptr(dp))
        total, k = np.full(1, 7, np.uint64), np.full(1, 7, np.uint32)
        o = _abi.ReachExtOut(None, 0, _ptr(total), None, None, None, _ptr(k))
        fn = _abi.lib().cls_reach_external
        assert fn(eng.h, C.byref(spec), eng.if_id("ext"), 3, C.byref(o), 0, None) == _abi.E_INVAL
        assert total[0] == 7 and k[0] == 7
        err = _abi.lib().cls_last_error(eng.h).decode()
        assert "2^36" in err and "N 1024" in err and "K 601" in err, err
    finally:
        eng.close()


def _rows_at_starts(c, ids, ext, starts, fam):
    """The sweep's rows built on the host, line-major over both directions:
    (src_if, dst_if, src, dst, proto, sport, dport)."""
    p, n = len(c["pr"]), rc.N_EP
    di, pi, si, ki = (x.ravel() for x in np.meshgrid(np.arange(2), np.arange(p), np.arange(n), np.arange(len(starts)),
                                                     indexing="ij"))
    ing = di == 1
    rem = xc.mapped(starts[ki]) if fam == 16 else starts[ki].astype(np.uint32)
    pod = c["addrs"][si]
    sel = ing[:, None] if fam == 16 else ing
    ext_if = np.full(len(si), ext, np.uint32)
    return (np.where(ing, ext_if, ids[si]), np.where(ing, ids[si], ext_if), np.where(sel, rem, pod),
            np.where(sel, pod, rem), c["pr"][pi], c["sp"][pi], c["dp"][pi])


@pytest.mark.parametrize("fam", [4, 16])
def test_consistent_with_the_batch_path(fam, engines):
    """cls_connect_batch over the same rows built on the host at the engine's
    class starts, run-length encoded, equals every output."""
    eng, ids, ext = engines(fam)
    c = rc.case(fam)
    starts = np.unique(np.concatenate([eng.addr_classes(x) for x in xc.bound_rules(c, ALL)])).astype(np.int64)
    v = eng.connect_batch(*_rows_at_starts(c, ids, ext, starts, fam))
    r = _sweep(eng, ids, ext, c)
    assert r["n_classes"] == len(starts)
    _check(r, xc.ranges_ref(v.reshape(2, len(c["pr"]), rc.N_EP, len(starts)), starts), "batch path")


@pytest.mark.parametrize("fam", [4, 16])
def test_after_an_acl_change(fam, engines):
    """One ACL deleted, one re-put: the classes come from the new snapshot and
    the sweep equals the oracle on the changed configuration."""
    eng, ids, ext = engines(fam, None, changed=True)
    c = rc.case(fam)
    starts, ref = _ref(fam, changed=True)
    before, ref0 = _ref(fam)
    assert len(starts) != len(before) or (starts != before).any()
    assert ref[0].tobytes() != ref0[0].tobytes()
    r = _sweep(eng, ids, ext, c)
    _check(r, ref, "changed configuration")
    assert r["n_classes"] == len(xc.class_starts(xc.bound_rules(dc.after(fam), ALL)))


def _dotted(a):
    return "%d.%d.%d.%d" % (a >> 24, a >> 16 & 255, a >> 8 & 255, a & 255)


def test_connection_external_equals_the_reference_calls():
    """ACLEngine.connection_external on a replayed renderer scenario plus an
    unregistered pod and one on another node: every line's ranges tile
    0 .. 0xFFFFFFFF, neighbours differ, and at every range's ends and at
    random addresses the oracle engine's connection_pod_to_internet /
    connection_internet_to_pod gives the range's action."""
    import oracle
    from scenario_replay import load_scenarios, replay
    from vpp_amd.renderer import api
    from vpp_amd.engine import ACLEngine, Engine
    test = [t for t in load_scenarios() if t["name"] == "TestCombinedRules"][0]
    ghost, remote = api.PodID("ghost", "default"), api.PodID("remote", "default")
    probes = [(0, 123, 80), (1, 123, 53), (0, 123, 22)]
    seen = {"gpu": [], "oracle": 0, "multi": 0}
    whole = [(0, 0xFFFFFFFF, 3)]
    rng = np.random.default_rng(9)

    def pods_of(engine):
        if remote not in engine.pods:
            engine.register_pod(remote, "10.9.9.9", True)
        return sorted((p for p in engine.pods if p != remote), key=lambda p: (p.namespace, p.name)) + [ghost, remote]

    def check_gpu(engine, calls):
        pods = pods_of(engine)
        res = engine.connection_external(pods, probes)
        assert set(res) == {(d, p, s) for d in BOTH for p in range(len(probes)) for s in range(len(pods))}
        for (d, p, s), mine in res.items():
            assert mine[0][0] == 0 and mine[-1][1] == 0xFFFFFFFF
            for a, b in zip(mine, mine[1:]):
                assert b[0] == a[1] + 1 and a[2] != b[2]
            if s >= len(pods) - 2:
                assert mine == whole                                  # unregistered; on another node
            seen["multi"] += len(mine) > 1
        one = engine.connection_external(pods, probes, dirs="ingress")
        assert one == {k: v for k, v in res.items() if k[0] == "ingress"}
        seen["gpu"].append(res)
        return engine.connection_batch(calls)

    def check_oracle(engine, calls):
        pods = pods_of(engine)
        for (d, p, s), mine in seen["gpu"][seen["oracle"]].items():
            for lo, hi, act in mine:
                for a in {lo, hi, int(rng.integers(lo, hi + 1))}:
                    got = (engine.connection_pod_to_internet(pods[s], _dotted(a), *probes[p]) if d == "egress" else
                           engine.connection_internet_to_pod(_dotted(a), pods[s], *probes[p]))
                    assert got == act, (d, p, s, a, got, act)
        seen["oracle"] += 1
        return [getattr(engine, {"ConnectionPodToPod": "connection_pod_to_pod",
                                 "ConnectionPodToInternet": "connection_pod_to_internet",
                                 "ConnectionInternetToPod": "connection_internet_to_pod"}[fn])(*args)
                for fn, args in calls]

    _, failures = replay(test, lambda contiv: ACLEngine(contiv, Engine()), check_conn=check_gpu)
    assert not failures, "\n".join(failures)
    _, failures = replay(test, oracle.OracleACLEngine, check_conn=check_oracle)
    assert not failures, "\n".join(failures)
    assert seen["oracle"] == len(seen["gpu"]) >= 2 and seen["multi"] > 0
    # an empty node output interface name: every pod fails before testConnection
    from vpp_amd.renderer.acl import ContivIfs
    eng = ACLEngine(ContivIfs(), Engine())
    try:
        pod = api.PodID("p", "default")
        eng.contiv.set_pod_if_name(pod, "tap1")
        eng.register_pod(pod, "10.1.1.1", False)
        res = eng.connection_external([pod, ghost], probes[:1], dirs="egress")
        assert res == {("egress", 0, 0): whole, ("egress", 0, 1): whole}
        # every line has a list of its own; an unknown direction is an error, as in Engine.reach_external
        res[("egress", 0, 0)].append(None)
        assert res[("egress", 0, 1)] == whole
        from vpp_amd._abi import ClsError
        for bad in ("sideways", ("egress", "out")):
            with pytest.raises(ClsError):
                eng.connection_external([pod], probes[:1], dirs=bad)
    finally:
        eng.engine.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_go_shims_reach_external(fam, tmp_path, engines):
    """go/shimtest/reachext (gcc): the sweep through clsg_reach_external_v4 /
    clsg_reach_external_v16, as the Go binding's ReachExternal calls them; its
    output files equal the Python call's."""
    if not os.path.exists(REACHEXT):
        subprocess.run(["make", "-s", "-C", os.path.dirname(REACHEXT)], check=True)
    c = rc.case(fam)
    assert c["ifs"][0] == xc.EXT_IF                       # reachext sweeps through the first interface
    eng, ids, ext = engines(fam)
    want = _sweep(eng, ids, ext, c)
    _check(want, _ref(fam)[1], "python")
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
    r = subprocess.run([REACHEXT, str(tmp_path), str(fam)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    shape = (2, len(c["pr"]), rc.N_EP)
    assert int(np.fromfile(tmp_path / "out_ext_n.bin", "<u8")[0]) == want["total"]
    assert (tmp_path / "out_ext_ranges.bin").read_bytes() == want["ranges"].tobytes()
    _same(np.fromfile(tmp_path / "out_ext_runs.bin", "<u4").reshape(shape), want["runs"], "runs")
    _same(np.fromfile(tmp_path / "out_ext_allow.bin", "<u8").reshape(shape), want["allow_addrs"], "allow_addrs")
    _same(np.fromfile(tmp_path / "out_ext_hist.bin", "<u8").reshape(shape[:2] + (4,)), want["hist"], "hist")
    assert int(np.fromfile(tmp_path / "out_ext_k.bin", "<u4")[0]) == want["n_classes"]
