"""The port sweep on the GPU (cls_reach_ports, Engine.reach_ports,
ACLEngine.connection_ports): per-pair port ranges over all 65,536 destination
ports.

The ranges -- maximal, in (src, dst, port_lo) order whatever the class
decomposition, the tiling, the evaluator and the form -- their total, the runs
and ALLOW ports per pair and the histogram must equal the numpy definition
(reach_ports_cases.ranges_ref) of the oracle's verdicts, bit for bit: of a
brute force over every port for six endpoints, of the oracle at the class
starts for all 37 (with random cells checked against the oracle directly),
with dummy classes that move every pair's rows across chunk, wave and group
boundaries, with tiles of 1,024 rows and with more classes than a tile has
rows, under every cap, in the device form, after an ACL change, through the
renderer-level call and the Go shims; and every refusal leaves its outputs
alone."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import reach_diff_cases as dc
import reach_ports_cases as pc
from test_gpu_reach import _same, _write_acls
from vpp_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHPORTS = os.path.join(ROOT, "go", "shimtest", "reachports")
SENTINEL = 0xA5
ALL = np.arange(rc.N_EP)


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


@functools.lru_cache(maxsize=None)
def _at_starts(fam, proto, eps=None, changed=False):
    """(class starts of the restatement, the oracle's verdicts at them) for
    endpoints eps (a tuple; None: all 37)."""
    c = dc.after(fam) if changed else rc.case(fam)
    e = ALL if eps is None else np.array(eps)
    starts = pc.class_starts(pc.bound_rules(c, e), proto)
    v = pc.oracle_at(fam, e, proto, starts, changed=changed)
    v.setflags(write=False)
    return starts, v


def _sweep(eng, ids, c, eps, proto, **kw):
    return eng.reach_ports(ids[eps], c["addrs"][eps], proto, pc.SPORT[proto], **kw)


def _check(r, ref, what, k=None):
    """A host-form ReachPorts against ranges_ref's tuple."""
    rec, total, runs, allow, hist = ref
    assert r.n_ranges == total, (what, r.n_ranges, total)
    assert r.ranges.dtype == _abi.PORT_RANGE and len(r.ranges) == len(rec), (what, len(r.ranges), len(rec))
    for f in ("src", "dst", "port_lo", "port_hi", "action", "zero"):
        _same(r.ranges[f], rec[f], "%s: ranges' %s" % (what, f))
    _same(r.runs, runs, what + ": runs")
    _same(r.allow_ports, allow, what + ": allow_ports")
    _same(r.hist, hist, what + ": hist")
    assert int(r.hist.sum()) == 65536 * runs.size, what
    if k is not None:
        assert r.n_classes == k, (what, r.n_classes, k)


def _equal(a, b, what):
    """Two host-form results, byte for byte (n_classes aside)."""
    assert a.n_ranges == b.n_ranges and a.ranges.tobytes() == b.ranges.tobytes(), what
    assert a.runs.tobytes() == b.runs.tobytes() and a.allow_ports.tobytes() == b.allow_ports.tobytes(), what
    assert a.hist.tobytes() == b.hist.tobytes(), what


@pytest.mark.parametrize("mode", ["auto", "classifier", "linear"])
@pytest.mark.parametrize("proto", [0, 1])
@pytest.mark.parametrize("fam", [4, 16])
def test_brute_force_over_all_ports(fam, proto, mode, engines):
    """Six endpoints x all 65,536 ports: everything the call returns equals
    the numpy definition of the oracle's brute force."""
    eng, ids = engines(fam)
    c = rc.case(fam)
    eps, v = pc.brute(fam, proto)
    k = len(pc.class_starts(pc.bound_rules(c, eps), proto))
    r = _sweep(eng, ids, c, eps, proto, mode=mode)
    _check(r, pc.ranges_ref(v), "brute force %s" % mode, k)
    assert int(r.hist.sum()) == 36 * 65536
    # the engine's classes: the sorted union of cls_port_classes over the bound ACLs
    union = np.unique(np.concatenate([eng.port_classes(x, proto) for x in pc.bound_rules(c, eps)]))
    assert r.n_classes == len(union)


@pytest.mark.parametrize("proto", [0, 1])
@pytest.mark.parametrize("fam", [4, 16])
def test_all_endpoints(fam, proto, engines):
    """All 37 endpoints (1,369 pairs, more than 100 chunks of rows, the global
    table on the pair launch) against the oracle at the class starts; 20,000
    random (pair, port) cells looked up in the ranges against the oracle
    directly."""
    eng, ids = engines(fam)
    c = rc.case(fam)
    starts, v = _at_starts(fam, proto)
    assert len(starts) * rc.N_EP ** 2 > 100 * 4096
    r = _sweep(eng, ids, c, ALL, proto)
    _check(r, pc.ranges_ref(v, starts), "37 endpoints", len(starts))
    rng = np.random.default_rng(77 + fam + proto)
    s, d = rng.integers(0, rc.N_EP, 20000), rng.integers(0, rc.N_EP, 20000)
    port = np.where(rng.random(20000) < 0.5, rng.integers(0, 65536, 20000),
                    rng.choice(starts, 20000) - rng.integers(0, 2, 20000)) & 0xFFFF
    want = pc.oracle_at(fam, ALL, proto, None, pairs=(s, d, port))
    _same(pc.lookup(r.ranges, rc.N_EP, s, d, port), want, "random cells")


def _dummy_rules(m, starts):
    """One rule without ports and m single-port TCP rules whose networks no
    endpoint has, on ports that add 2 m classes."""
    from vpp_amd import model as M
    rules = [M.icmp_rule(M.PERMIT, "203.0.113.0/24", "203.0.113.0/24")]
    taken, p = set(int(x) for x in starts), 30001
    while len(rules) < m + 1:
        if not {p - 1, p, p + 1, p + 2} & taken:
            rules.append(M.l4_rule(M.PERMIT, "203.0.113.0/24", "203.0.113.0/24", "tcp", 0, 65535, p, p))
            taken |= {p, p + 1}
        p += 7
    return rules


@functools.lru_cache(maxsize=None)
def _dummy_ref(fam, eps):
    """The oracle at the class starts with an ACL that never matches bound
    outbound to the unbound interface (a bound ACL that matches nothing
    denies, where no ACL permits)."""
    import oracle
    c = rc.case(fam)
    free = c["ifs"][c["at"][3]]
    assert c["bind"][free] == [None, None] and 3 in eps
    names = sorted(c["by_name"]) + ["dummy"]
    by_name = dict(c["by_name"], dummy=_dummy_rules(0, []))
    bind = dict(c["bind"], **{free: [None, "dummy"]})
    tabs = [oracle.FastTable(oracle.rules_to_c(by_name[x])) for x in names]
    if_in = [names.index(bind[f][0]) if bind[f][0] else -1 for f in c["ifs"]]
    if_out = [names.index(bind[f][1]) if bind[f][1] else -1 for f in c["ifs"]]
    e = np.array(eps)
    starts = pc.class_starts(pc.bound_rules(c, e), 0)
    s, d, p = (x.ravel() for x in np.meshgrid(np.arange(len(e)), np.arange(len(e)), np.arange(len(starts)),
                                              indexing="ij"))
    tr = {"src": c["addrs"][e[s]], "dst": c["addrs"][e[d]], "proto": np.zeros(len(s), np.uint8),
          "sport": np.full(len(s), pc.SPORT[0], np.uint16), "dport": starts[p].astype(np.uint16)}
    v = oracle.connect_fast(tabs, if_in, if_out, c["at"][e[s]], c["at"][e[d]], tr, af=fam)
    return starts, pc.ranges_ref(v.reshape(len(e), len(e), len(starts)), starts)


@pytest.mark.parametrize("n", [36, 5])
@pytest.mark.parametrize("fam", [4, 16])
def test_row_offsets_move_with_dummy_classes(fam, n):
    """An extra ACL of m = 0..3 single-port rules that match nothing: K grows
    by 2 m, so every pair's first row moves across chunk, wave and
    group-of-four boundaries; merging removes the dummy boundaries, so all but
    n_classes is identical across m and equals the reference."""
    from vpp_amd.engine import Engine
    c = rc.case(fam)
    # (endpoint 3 is on the unbound interface; the rest of the five from the brute force's six)
    eps = tuple(range(36)) if n == 36 else (3,) + tuple(int(x) for x in pc.brute_endpoints(fam, 0) if x != 3)[:4]
    starts, ref = _dummy_ref(fam, eps)
    e = np.array(eps)
    eng = Engine()
    try:
        ids = rc.install(eng, c)
        free = c["ifs"][c["at"][3]]
        first = None
        for m in range(4):
            assert eng.acl_put("dummy", _dummy_rules(m, starts), [], [free]) == 0
            r = _sweep(eng, ids, c, e, 0)
            _check(r, ref, "m = %d" % m, len(starts) + 2 * m)
            first = first or r
            _equal(r, first, "m = %d against m = 0" % m)
    finally:
        eng.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_tiles_of_1024_rows(fam, engines):
    """reach_tile 1024 (a few pairs per tile) and the default (one tile) give
    byte-identical outputs."""
    c = rc.case(fam)
    (eng, ids), (small, ids_s) = engines(fam), engines(fam, 1024)
    a, b = _sweep(eng, ids, c, ALL, 0), _sweep(small, ids_s, c, ALL, 0)
    assert a.n_classes == b.n_classes and 1 <= 1024 // a.n_classes < 8
    _equal(a, b, "reach_tile 1024 against the default")
    starts, v = _at_starts(fam, 0)
    _check(b, pc.ranges_ref(v, starts), "reach_tile 1024", len(starts))


def test_more_classes_than_a_tile():
    """K > reach_tile = 1024: a tile is one pair's K rows.  Three endpoints
    over one ACL of many distinct port ranges, against the oracle at the class
    starts."""
    import oracle
    from aclgen import many_ports_acl
    from vpp_amd.engine import Engine
    rules, _ = many_ports_acl(11, n_rules=1800)
    starts = pc.class_starts([rules], 0)
    assert len(starts) > 1024

    def ip4(cidr):
        a, b, c_, d = (int(x) for x in cidr.split("/")[0].split("."))
        return a << 24 | b << 16 | c_ << 8 | d
    tcp = [r for r in rules if r.matches.ip_rule.tcp is not None]
    addrs = np.array([ip4(tcp[0].matches.ip_rule.ip.source_network), ip4(tcp[0].matches.ip_rule.ip.destination_network),
                      ip4(tcp[1].matches.ip_rule.ip.source_network)], np.uint32)
    at = np.array([0, 1, 0])
    s, d, p = (x.ravel() for x in np.meshgrid(np.arange(3), np.arange(3), np.arange(len(starts)), indexing="ij"))
    tr = {"src": addrs[s], "dst": addrs[d], "proto": np.zeros(len(s), np.uint8),
          "sport": np.full(len(s), 40000, np.uint16), "dport": starts[p].astype(np.uint16)}
    v = oracle.connect_fast([oracle.FastTable(oracle.rules_to_c(rules))], [0, -1], [-1, 0], at[s], at[d], tr)
    ref = pc.ranges_ref(v.reshape(3, 3, len(starts)), starts)
    assert ref[2].max() > 1
    got = []
    for tile in (1024, None):
        eng = Engine(options={"reach_tile": tile} if tile else None)
        try:
            assert eng.acl_put("big", rules, ["ifa"], ["ifb"]) == 0
            ids = np.array([eng.if_id("ifa"), eng.if_id("ifb")], np.uint32)[at]
            got.append(eng.reach_ports(ids, addrs, 0, 40000))
            _check(got[-1], ref, "K > tile, reach_tile %s" % tile, len(starts))
        finally:
            eng.close()
    _equal(got[0], got[1], "K > tile against one tile")


class _Raw:
    """cls_reach_ports through ctypes on sentinel-filled host outputs."""

    def __init__(self, eng, c, ids, eps, proto, n_rec):
        from vpp_amd.engine import _ptr
        self.eng, self.ptr = eng, _ptr
        self.ids = np.ascontiguousarray(ids[eps], np.uint32)
        fam16 = c["fam"] == 16
        self.addrs = np.ascontiguousarray(c["addrs"][eps], np.uint8 if fam16 else np.uint32)
        self.pr, self.sp = np.array([proto, proto], np.uint8), np.array([pc.SPORT[proto]] * 2, np.uint16)
        self.N = N = len(self.ids)
        self.fields = dict(af=_abi.AF_V16 if fam16 else _abi.AF_V4, n_endpoints=N, if_id=_ptr(self.ids),
                           addr4=None if fam16 else _ptr(self.addrs), addr16=_ptr(self.addrs) if fam16 else None,
                           n_probes=1, proto=_ptr(self.pr), sport=_ptr(self.sp), dport=None)
        self.out = dict(ranges=np.zeros(n_rec, _abi.PORT_RANGE), n_ranges=np.zeros(1, np.uint64),
                        runs_out=np.zeros((N, N), np.uint32), allow_ports_out=np.zeros((N, N), np.uint32),
                        hist_out=np.zeros(4, np.uint64), n_classes=np.zeros(1, np.uint32))
        self.fill()

    def fill(self):
        for a in self.out.values():
            a.view(np.uint8).reshape(-1)[:] = SENTINEL

    def untouched(self, *names):
        return all((self.out[k].view(np.uint8) == SENTINEL).all() for k in (names or self.out))

    def spec(self, **kw):
        f = dict(self.fields, **kw)
        return _abi.ReachSpec(*[f[k] for k, _ in _abi.ReachSpec._fields_])

    def call(self, spec=None, cap=None, flags=0, **ptrs):
        """ptrs: output name -> replacement (None: leave it out)."""
        o = {k: self.ptr(v) for k, v in self.out.items()}
        o.update(ptrs)
        cap = len(self.out["ranges"]) if cap is None else cap
        st = _abi.ReachPortsOut(o["ranges"], cap, o["n_ranges"], o["runs_out"], o["allow_ports_out"], o["hist_out"],
                                o["n_classes"])
        return _abi.lib().cls_reach_ports(self.eng.h, C.byref(spec or self.spec()), C.byref(st), flags, None)


@pytest.mark.parametrize("fam", [4, 16])
def test_cap(fam, engines):
    """cap 1, one that ends inside a pair of the first tile, one that ends in
    a later tile, the total and more: the first min(total, cap) records, the
    sentinels behind them untouched, the total unchanged."""
    small, ids = engines(fam, 8192)
    c = rc.case(fam)
    starts, v = _at_starts(fam, 0)
    rec, total, runs, allow, hist = pc.ranges_ref(v, starts)
    per_tile = 8192 // len(starts)
    in_tile0 = int(runs.ravel()[:per_tile].sum())
    multi = int(np.flatnonzero(runs.ravel() > 1)[0])
    mid_pair = int(runs.ravel()[:multi].sum()) + 1            # ends inside the first pair with several ranges
    assert multi < per_tile and 1 < mid_pair < in_tile0 < total
    later = int(runs.ravel()[:700].sum()) + 1
    raw = _Raw(small, c, ids, ALL, 0, total + 8)
    for cap in (1, mid_pair, later, total, total + 8):
        raw.fill()
        assert raw.call(cap=cap) == 0, cap
        n = min(cap, total)
        assert int(raw.out["n_ranges"][0]) == total, cap
        assert raw.out["ranges"][:n].tobytes() == rec[:n].tobytes(), cap
        assert (raw.out["ranges"][n:].view(np.uint8) == SENTINEL).all(), cap
        _same(raw.out["runs_out"], runs, "cap %d: runs" % cap)
        _same(raw.out["hist_out"], hist, "cap %d: hist" % cap)
        assert int(raw.out["n_classes"][0]) == len(starts)
    # the Python call: cap cuts the records, cap 0 asks for none
    r = _sweep(small, ids, c, ALL, 0, cap=later)
    assert r.n_ranges == total and r.ranges.tobytes() == rec[:later].tobytes()
    r = _sweep(small, ids, c, ALL, 0, cap=0)
    assert r.ranges is None and r.n_ranges == total


@pytest.mark.parametrize("fam", [4, 16])
def test_device_form(fam, engines):
    """torch outputs on a side stream equal the host form; n_classes is set on
    return; records past the total stay; each misaligned pointer is refused."""
    import torch
    eng, ids = engines(fam, 8192)
    c = rc.case(fam)
    host = _sweep(eng, ids, c, ALL, 0)
    cap = host.n_ranges + 5
    side = torch.cuda.Stream()
    rg = torch.full((cap, 4), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r = _sweep(eng, ids, c, ALL, 0, out=(rg, None, None, None, None), stream=side)
    assert r.n_classes == host.n_classes and r.ranges is rg
    side.synchronize()
    assert int(r.n_ranges.item()) == host.n_ranges
    got = rg.cpu().numpy()
    assert got[:host.n_ranges].tobytes() == host.ranges.tobytes()
    assert (got[host.n_ranges:] == -1).all()
    _same(r.runs.cpu().numpy().view(np.uint32), host.runs, "device runs")
    _same(r.allow_ports.cpu().numpy().view(np.uint32), host.allow_ports, "device allow_ports")
    _same(r.hist.cpu().numpy().view(np.uint64), host.hist, "device hist")
    # a device cap below the total
    few = torch.full((7, 4), -1, dtype=torch.int32, device="cuda")
    r2 = _sweep(eng, ids, c, ALL, 0, out=(few, None, None, None, None))
    torch.cuda.synchronize()
    assert int(r2.n_ranges.item()) == host.n_ranges and few.cpu().numpy().tobytes() == host.ranges[:7].tobytes()
    # misaligned device pointers
    raw = _Raw(eng, c, ids, ALL, 0, 1)
    N = rc.N_EP
    d = dict(ranges=torch.zeros(16 * cap + 16, dtype=torch.uint8, device="cuda"),
             n_ranges=torch.zeros(2, dtype=torch.int64, device="cuda"),
             runs_out=torch.zeros(N * N + 1, dtype=torch.int32, device="cuda"),
             allow_ports_out=torch.zeros(N * N + 1, dtype=torch.int32, device="cuda"),
             hist_out=torch.zeros(5, dtype=torch.int64, device="cuda"))
    ok = {k: t.data_ptr() for k, t in d.items()}
    for name, off in (("ranges", 8), ("n_ranges", 4), ("runs_out", 2), ("allow_ports_out", 1), ("hist_out", 4)):
        raw.fill()
        assert raw.call(cap=cap, flags=_abi.F_DEVICE, **dict(ok, **{name: ok[name] + off})) == _abi.E_INVAL, name
        torch.cuda.synchronize()
        assert raw.untouched("n_classes") and not any(bool(t.any()) for t in d.values()), name
    assert raw.call(cap=cap, flags=_abi.F_DEVICE, **ok) == 0
    torch.cuda.synchronize()
    assert int(d["n_ranges"][0].item()) == host.n_ranges and int(raw.out["n_classes"][0]) == host.n_classes


def test_refusals_leave_the_outputs_alone(engines):
    """Every CLS_E_INVAL of cls_reach_ports, on sentinel-filled outputs; the
    next valid call still matches."""
    eng, ids = engines(4)
    c = rc.case(4)
    eps, v = pc.brute(4, 0)
    ref = pc.ranges_ref(v)
    raw = _Raw(eng, c, ids, eps, 0, ref[1])
    bad = raw.ids.copy()
    bad[3] = 1 << 20
    wide = np.full(1 << 18, raw.ids[0], np.uint32)
    wide_addr = np.zeros(1 << 18, np.uint32)
    none = dict(ranges=None, n_ranges=None, runs_out=None, allow_ports_out=None, hist_out=None)
    refused = {
        "n_probes 2": lambda: raw.call(raw.spec(n_probes=2)),
        "n_probes 0": lambda: raw.call(raw.spec(n_probes=0)),
        "N = 0": lambda: raw.call(raw.spec(n_endpoints=0)),
        "bad af": lambda: raw.call(raw.spec(af=6)),
        "NULL if_id": lambda: raw.call(raw.spec(if_id=None)),
        "NULL addr4": lambda: raw.call(raw.spec(addr4=None)),
        "NULL proto": lambda: raw.call(raw.spec(proto=None)),
        "NULL sport": lambda: raw.call(raw.spec(sport=None)),
        "CLS_F_COUNT": lambda: raw.call(flags=_abi.F_COUNT),
        "CLS_F_NO_VERDICT": lambda: raw.call(flags=_abi.F_NO_VERDICT),
        "unknown interface id": lambda: raw.call(raw.spec(if_id=raw.ptr(bad))),
        "no outputs": lambda: raw.call(**none),
        "ranges without n_ranges": lambda: raw.call(n_ranges=None),
        "cap 0": lambda: raw.call(cap=0),
        "N > 2^18": lambda: raw.call(raw.spec(n_endpoints=(1 << 18) + 1)),
        "K N^2 > 2^36": lambda: raw.call(raw.spec(n_endpoints=1 << 18, if_id=raw.ptr(wide),
                                                  addr4=raw.ptr(wide_addr))),
    }
    for what, f in refused.items():
        raw.fill()
        assert f() == _abi.E_INVAL, what
        assert raw.untouched(), what
    err = _abi.lib().cls_last_error(eng.h).decode()
    assert "2^36" in err and "N %d" % (1 << 18) in err and "K " in err, err
    assert int(err.split("K ")[1].split()[0]) >= 2
    _check(_sweep(eng, ids, c, eps, 0), ref, "after the refusals")
    # a NULL dport is what the call takes; one output alone is enough
    raw.fill()
    assert raw.call(**dict(none, hist_out=raw.ptr(raw.out["hist_out"]))) == 0
    _same(raw.out["hist_out"], ref[4], "hist alone")
    assert raw.untouched("ranges", "n_ranges", "runs_out", "allow_ports_out")


@pytest.mark.parametrize("proto", [2, 47])
@pytest.mark.parametrize("fam", [4, 16])
def test_protocols_without_ports(fam, proto, engines):
    """ICMP and protocol 47: no rule tests the port, so K = 1 and every pair
    has the one range 0..65535 with the matrix's action."""
    eng, ids = engines(fam)
    c = rc.case(fam)
    r = _sweep(eng, ids, c, ALL, proto)
    m, _, _ = eng.reach_matrix(ids, c["addrs"], [proto], [pc.SPORT[proto]], [0], hist=False, allow=False)
    n = rc.N_EP
    assert r.n_classes == 1 and r.n_ranges == n * n and (r.runs == 1).all()
    _same(r.ranges["src"] * n + r.ranges["dst"], np.arange(n * n), "pairs")
    assert (r.ranges["port_lo"] == 0).all() and (r.ranges["port_hi"] == 65535).all()
    _same(r.ranges["action"].reshape(n, n), m[0], "actions")
    _same(r.allow_ports, np.where(m[0] == rc.ALLOW, 65536, 0), "allow_ports")
    _same(r.hist, np.bincount(m[0].ravel(), minlength=4) * 65536, "hist")


@pytest.mark.parametrize("fam", [4, 16])
def test_consistent_with_the_matrix(fam, engines):
    """A table port, 0 and 65535 looked up in the ranges equal
    cls_reach_matrix with that probe."""
    eng, ids = engines(fam)
    c = rc.case(fam)
    r = _sweep(eng, ids, c, ALL, 0)
    ports = [int(c["dp"][0]), 0, 65535]
    m, _, _ = eng.reach_matrix(ids, c["addrs"], [0] * 3, [pc.SPORT[0]] * 3, ports, hist=False, allow=False)
    s, d = (x.ravel() for x in np.meshgrid(ALL, ALL, indexing="ij"))
    for k, port in enumerate(ports):
        _same(pc.lookup(r.ranges, rc.N_EP, s, d, np.full(len(s), port)), m[k].ravel(), "port %d" % port)


@pytest.mark.parametrize("fam", [4, 16])
def test_after_an_acl_change(fam, engines):
    """One ACL deleted, one re-put: the classes come from the new snapshot and
    the sweep equals the oracle on the changed configuration."""
    eng, ids = engines(fam, None, changed=True)
    c = rc.case(fam)
    starts, v = _at_starts(fam, 0, changed=True)
    before, _ = _at_starts(fam, 0)
    assert len(starts) != len(before) or (starts != before).any()
    ref = pc.ranges_ref(v, starts)
    assert ref[0].tobytes() != pc.ranges_ref(_at_starts(fam, 0)[1], before)[0].tobytes()
    _check(_sweep(eng, ids, c, ALL, 0), ref, "changed configuration", len(starts))


def test_connection_ports_equals_pod_to_pod():
    """ACLEngine.connection_ports on a replayed renderer scenario plus an
    unregistered pod: the ranges of every pair tile 0..65535, neighbours
    differ, and at every range's ends the oracle engine's
    connection_pod_to_pod gives the range's action."""
    import oracle
    from scenario_replay import load_scenarios, replay
    from vpp_amd.renderer import api
    from vpp_amd.engine import ACLEngine, Engine
    test = [t for t in load_scenarios() if t["name"] == "TestCombinedRules"][0]
    ghost = api.PodID("ghost", "default")
    seen = {"gpu": [], "oracle": 0, "multi": 0}

    def pods_of(engine):
        return sorted(engine.pods, key=lambda p: (p.namespace, p.name)) + [ghost]

    def check_gpu(engine, calls):
        pods = pods_of(engine)
        ranges, runs = engine.connection_ports(pods, 0, 123)
        n = len(pods)
        assert runs.shape == (n, n) and runs.sum() == len(ranges)
        assert ranges == sorted(ranges)
        for s in range(n):
            for d in range(n):
                mine = [r for r in ranges if r[0] == s and r[1] == d]
                assert len(mine) == runs[s, d] and mine[0][2] == 0 and mine[-1][3] == 65535
                for a, b in zip(mine, mine[1:]):
                    assert b[2] == a[3] + 1 and a[4] != b[4]
                if s == n - 1 or d == n - 1:
                    assert mine == [(s, d, 0, 65535, 3)]                    # the unregistered pod
        seen["multi"] += int((runs > 1).sum())
        seen["gpu"].append(ranges)
        return engine.connection_batch(calls)

    def check_oracle(engine, calls):
        pods = pods_of(engine)
        for s, d, lo, hi, act in seen["gpu"][seen["oracle"]]:
            for port in {lo, hi, (lo + hi) // 2}:
                assert engine.connection_pod_to_pod(pods[s], pods[d], 0, 123, port) == act, (s, d, port)
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
    eng = ACLEngine(None, Engine())
    try:
        ranges, runs = eng.connection_ports([ghost, ghost], 0, 1)
        assert ranges == [(s, d, 0, 65535, 3) for s in range(2) for d in range(2)] and (runs == 1).all()
    finally:
        eng.engine.close()


@pytest.mark.parametrize("fam", [4, 16])
def test_go_shims_reach_ports(fam, tmp_path, engines):
    """go/shimtest/reachports (gcc): the sweep through clsg_reach_ports_v4 /
    clsg_reach_ports_v16, as the Go binding's ReachPorts calls them; its
    output files equal the Python call's."""
    if not os.path.exists(REACHPORTS):
        subprocess.run(["make", "-s", "-C", os.path.dirname(REACHPORTS)], check=True)
    c = rc.case(fam)
    eng, ids = engines(fam)
    want = _sweep(eng, ids, c, ALL, 0)
    starts, v = _at_starts(fam, 0)
    _check(want, pc.ranges_ref(v, starts), "python", len(starts))
    _write_acls(tmp_path / "acls.txt", c)
    (tmp_path / "ifs.txt").write_text("\n".join(c["ifs"]) + "\n")
    with open(tmp_path / "reach.bin", "wb") as f:
        f.write(np.array([len(c["at"]), 1], "<u4").tobytes())
        f.write(np.ascontiguousarray(c["at"], "<u4").tobytes())
        f.write(np.ascontiguousarray(c["addrs"], "<u4" if fam == 4 else np.uint8).tobytes())
        f.write(np.array([0], np.uint8).tobytes())
        f.write(np.array([pc.SPORT[0]], "<u2").tobytes())
        f.write(np.array([0], "<u2").tobytes())
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(
        [os.path.join(ROOT, "vpp_amd")] + [x for x in [os.environ.get("LD_LIBRARY_PATH")] if x]))
    r = subprocess.run([REACHPORTS, str(tmp_path), str(fam)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    n = rc.N_EP
    assert int(np.fromfile(tmp_path / "out_ports_n.bin", "<u8")[0]) == want.n_ranges
    assert (tmp_path / "out_ports_ranges.bin").read_bytes() == want.ranges.tobytes()
    _same(np.fromfile(tmp_path / "out_ports_runs.bin", "<u4").reshape(n, n), want.runs, "runs")
    _same(np.fromfile(tmp_path / "out_ports_allow.bin", "<u4").reshape(n, n), want.allow_ports, "allow_ports")
    _same(np.fromfile(tmp_path / "out_ports_hist.bin", "<u8"), want.hist, "hist")
    assert int(np.fromfile(tmp_path / "out_ports_k.bin", "<u4")[0]) == want.n_classes
