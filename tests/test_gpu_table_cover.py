"""GPU tests of the rule coverage sweep (cls_table_cover, Engine.table_cover,
ACLEngine.acl_coverage, the Go shims).

Bar: bit-exact equality with cover_cases.cover_ref -- the OpenMP oracle over
the representative packets of every cell, reduced with numpy -- whose own
soundness test_table_cover_cpu.py states without classes.  Every table stays
at or below 2^22 cells."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cover_cases as cc
from aclgen import random_acl, random_acl16, single_port_acl
from vpp_amd import _abi
from vpp_amd import model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLECOVER = os.path.join(ROOT, "go", "shimtest", "tablecover")
FIELDS = ("src", "dst", "proto", "dport")


@pytest.fixture(scope="module")
def eng():
    from vpp_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _cover(eng, rules, af=4, mode="auto", want=None, what=""):
    t = eng.put_table("cover", rules)
    try:
        got = eng.table_cover(t, af=af, mode=mode)
    finally:
        eng.del_table(t)
    if want is not None:
        cc.assert_equal(got, want, what)
    return got


# ---- constructed shadows ------------------------------------------------------

@pytest.mark.parametrize("af", [4, 16])
def test_constructed_shadows(eng, af):
    rules, dead = cc.shadow_acl()
    names = [r.rule_name for r in rules]
    got = _cover(eng, rules, af, want=cc.cover_ref(rules, af), what="shadows af %d" % af)
    assert [names[k] for k in np.flatnonzero(got["live"][:-1] == 0)] == dead
    assert got["live"][-1] == 0 and got["n_dead"] == len(dead)
    w = got["witness"]
    assert w[names.index("tcp_other_only")]["proto"] == 3
    assert tuple(w[names.index("icmp")]) == (0, 0, 0, 2, 1, 0)
    assert tuple(w[names.index("macip")]) == (0, 0, 0, 0, 1, 0)
    assert tuple(w[names.index("whole24")]) == (0, 0, 0, 0, 0, 0)


# ---- random parity ------------------------------------------------------------

@pytest.mark.parametrize("mode", ["auto", "linear"])
@pytest.mark.parametrize("af", [4, 16])
@pytest.mark.parametrize("weird", [0.0, 0.3])
@pytest.mark.parametrize("n", [5, 80, 400])
def test_random_parity(eng, n, weird, af, mode):
    gen = random_acl16 if af == 16 else random_acl
    rules = cc.shadowed_tail(gen(n * 3 + int(weird * 10) + 1, n, weird)[0], n)
    ref = cc.cover_ref(rules, af)
    assert ref["n_dead"] >= 1 and int(ref["live"].sum()) >= 2     # no vacuous pass
    _cover(eng, rules, af, mode, want=ref, what="random %d %.1f af %d %s" % (n, weird, af, mode))


# ---- evaluator independence ---------------------------------------------------

@pytest.mark.parametrize("af", [4, 16])
@pytest.mark.parametrize("opts", [{"orient": "src"}, {"orient": "dst"}, {"list_mode": "0"}, {"list_mode": "1"},
                                  {"list_mode": "3"}], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_evaluator_independence(eng, libopt, opts, af):
    """The result is the same whichever image the compiler is forced to build."""
    rules = cc.shadowed_tail(random_acl(77, 120, 0.1)[0], 5)
    want = cc.cover_ref(rules, af)
    for k, v in opts.items():
        libopt.set(k, v, eng)
    _cover(eng, rules, af, want=want, what=str(opts))


@pytest.mark.parametrize("af", [4, 16])
@pytest.mark.parametrize("trie,wide", [("1", "0"), ("1", "1"), ("0", "1")])
def test_trie_and_wide_cells(eng, libopt, trie, wide, af):
    rules = cc.shadowed_tail(single_port_acl(22, 300, n_prefixes=24)[0], 3)
    want = cc.cover_ref(rules, af)
    libopt.set("orient", "src", eng)
    libopt.set("trie", trie, eng)
    libopt.set("wide", wide, eng)
    _cover(eng, rules, af, want=want, what="trie %s wide %s" % (trie, wide))


def test_v4_and_v16_sweeps_agree(eng):
    rules = cc.shadowed_tail(random_acl(31, 150, 0.0)[0], 8)
    a, b = _cover(eng, rules, 4), _cover(eng, rules, 16)
    cc.assert_equal(a, b, "v4 against v16")
    cc.assert_equal(a, cc.cover_ref(rules, 4), "v4")


# ---- tile edges ---------------------------------------------------------------

def _edge_table():
    """An 80-rule list plus, placed by arithmetic on its class starts: `last`,
    a /32 -> /32 single-port rule whose only cell is the last cell of a 1024
    tile; `first`, one whose only cell is the first cell of a tile; `end`, one
    whose only cell is the last cell of the sweep; `wide`, a rule whose cells
    are one run over three tiles.  Each single-cell rule follows a rule of the
    same networks with an empty UDP range, which takes their protocols above 2
    and adds no class."""
    base = random_acl(12, 80, 0.0)[0]
    wide = cc._l4("wide", "1.0.0.0/8", "tcp", 80, 80, dst="garbage")      # FAILURE for every packet from 1/8
    S, D = cc.side_starts([wide] + base, 0), cc.side_starts(base, 1)
    _, _, kt, ku = cc.columns(base)
    Pt = cc.port_starts([base], 0)
    top = 0xFFFFFFFF
    assert top not in S and top not in D
    # the classes once all three rules are in: two starts per /32 (one for 255.255.255.255) and per port
    kd, t = len(D) + 5, kt + 2 * 2 + ku + 2

    def fresh(v):
        """Values x with x, x + 1 not in v and not next to one."""
        return [int(a) + 2 for a, b in zip(v[:-1], v[1:]) if b - a > 5]

    def places(target, before):
        """Every (a, b, p) whose cell is `target` modulo 1024 with `before` new /32s and ports below each."""
        out = []
        for a in fresh(S):
            s = int(np.searchsorted(S, a)) + 2 * before
            for b in fresh(D):
                d = int(np.searchsorted(D, b)) + 2 * before
                for p in fresh(Pt):
                    j = int(np.searchsorted(Pt, p)) + 2 * before
                    if ((s * kd + d) * t + j) % 1024 == target:
                        out.append((a, b, p))
        return out

    ip = lambda x: "%d.%d.%d.%d/32" % (x >> 24, x >> 16 & 255, x >> 8 & 255, x & 255)
    pairs = [(x, y) for x in places(1023, 0) for y in places(0, 1) if all(v > u + 1 for u, v in zip(x, y))]
    assert pairs, "no placement"
    (a1, b1, p1), (a2, b2, p2) = pairs[0]
    extra = []
    for name, a, b, lo, hi in (("last", a1, b1, p1, p1), ("first", a2, b2, p2, p2), ("end", top, top, 9, 8)):
        extra.append(cc._l4("take3_" + name, ip(a), "udp", 9, 8, dst=ip(b)))
        extra.append(cc._l4(name, ip(a), "tcp", lo, hi, dst=ip(b)))
    # `end` keeps its protocols above 2: its only cell is the sweep's last column
    del extra[4]
    return [wide] + extra + base


def test_tile_edges(eng):
    rules = _edge_table()
    names = [r.rule_name for r in rules]
    ref = cc.cover_ref(rules)
    (ks, kd, kt, ku), n_cells = cc.dims(rules)
    t = kt + ku + 2
    assert t & (t - 1) and n_cells % 1024 and n_cells > 4096
    hit = cc.oracle_rules(rules, cc.cells(rules))
    at = {n: np.flatnonzero(hit == names.index(n)) for n in ("last", "first", "end", "wide")}
    assert len(at["last"]) == 1 and at["last"][0] % 1024 == 1023
    assert len(at["first"]) == 1 and at["first"][0] % 1024 == 0
    assert len(at["end"]) == 1 and at["end"][0] == n_cells - 1
    run = at["wide"]
    assert np.all(np.diff(run) == 1) and run[-1] // 1024 - run[0] // 1024 >= 2     # one run over three tiles
    tb = eng.put_table("edges", rules)
    try:
        for tile in (1024, 2048, (n_cells + 1023) & ~1023, 1 << 22, None):
            eng.set_option("cover_tile", tile)
            for af in (4, 16):
                for mode in ("auto", "linear"):
                    got = eng.table_cover(tb, af=af, mode=mode)
                    cc.assert_equal(got, ref if af == 4 else cc.cover_ref(rules, 16), "tile %s af %d %s" % (tile, af, mode))
    finally:
        eng.set_option("cover_tile", None)
        eng.del_table(tb)


def test_cover_tile_option(eng):
    from vpp_amd._abi import ClsError
    for bad in (1023, (1 << 30) + 1, -1):
        with pytest.raises(ClsError):
            eng.set_option("cover_tile", bad)
    eng.set_option("cover_tile", 1025)      # rounded up to 2048
    eng.set_option("cover_tile", None)


# ---- degenerate shapes --------------------------------------------------------

@pytest.mark.parametrize("af", [4, 16])
def test_degenerate_shapes(eng, af):
    # R = 0: only the default, at the least packet of all
    got = _cover(eng, [], af, want=cc.cover_ref([], af), what="R = 0")
    assert got["dims"] == (1, 1, 1, 1) and got["n_cells"] == 4 and got["n_dead"] == 0
    assert got["live"].tolist() == [1] and tuple(got["witness"][0]) == (0, 0, 0, 0, 1, 0)
    # a single allow-all rule (no sections: every protocol): the default is dead
    allow = [M.Rule(actions=M.Actions(M.PERMIT), matches=M.Matches(ip_rule=M.IpRule(ip=M.Ip())))]
    ref = cc.cover_ref(allow, af)
    assert ref["live"].tolist() == [1, 0]
    got = _cover(eng, allow, af, want=ref, what="allow-all")
    assert got["n_dead"] == 0 and got["cells"].tolist() == [4, 0]
    # Ks = Kd = 1 with 300 port classes
    ports = [cc._l4("p%d" % i, "", "tcp" if i % 2 else "udp", 100 * i, 100 * i + 49) for i in range(1, 151)]
    ref = cc.cover_ref(ports, af)
    assert ref["dims"][:2] == (1, 1) and ref["dims"][2] + ref["dims"][3] >= 300
    _cover(eng, ports, af, want=ref, what="Ks = Kd = 1")
    # Kt = Ku = 1
    nets = [cc._l4("n%d" % i, "10.%d.0.0/16" % i, "tcp", 0, 65535, dst="10.%d.0.0/%d" % (i % 7, 8 + i % 9))
            for i in range(40)]
    ref = cc.cover_ref(nets, af)
    assert ref["dims"][2:] == (1, 1)
    _cover(eng, nets, af, want=ref, what="Kt = Ku = 1")


@pytest.mark.parametrize("af", [4, 16])
def test_more_rules_than_the_folds_lds_bins(eng, af):
    """cover_fold counts in per-workgroup LDS bins up to 15,360 rules and in
    global memory above: 15,400 two-port TCP rules (one cell each, runs of one
    and two cells), a duplicate, and the default's long runs."""
    rules = [cc._l4("p%d" % i, "", "tcp", 4 * i, 4 * i + 1) for i in range(15400)]
    rules.append(cc._l4("dup", "", "tcp", 400, 401))
    ref = cc.cover_ref(rules, af)
    assert len(rules) + 1 > 15360 and ref["n_dead"] == 1 and ref["live"][-1] == 1
    for tile in (2048, None):
        eng.set_option("cover_tile", tile)
        try:
            _cover(eng, rules, af, want=ref, what="15401 rules, tile %s" % tile)
        finally:
            eng.set_option("cover_tile", None)


# ---- consistency with the shipped paths ---------------------------------------

@pytest.mark.parametrize("af", [4, 16])
def test_consistent_with_classify(eng, af):
    rules = cc.shadowed_tail((random_acl16 if af == 16 else random_acl)(9, 100, 0.2)[0], 4)
    tb = eng.put_table("consistent", rules)
    try:
        got = eng.table_cover(tb, af=af)
        w = got["witness"]
        k = np.flatnonzero(got["live"])
        conv = cc.mapped16 if af == 16 else (lambda a: np.ascontiguousarray(a, np.uint32))
        _, own = eng.classify_rules(tb, conv(w["src"][k]), conv(w["dst"][k]), np.ascontiguousarray(w["dport"][k]),
                                    np.ascontiguousarray(w["proto"][k]))
        assert np.array_equal(own, k)                             # every witness hits its own rule
        c = cc.cells(rules)
        _, ctr = eng.classify(tb, conv(c["src"]), conv(c["dst"]), c["dport"], c["proto"])
        assert np.array_equal(ctr, got["cells"]) and int(ctr.sum()) == got["n_cells"]
    finally:
        eng.del_table(tb)


# ---- device form ----------------------------------------------------------------

def test_device_form(eng):
    """torch outputs inside 64 padding elements on a side stream equal the
    host form and leave the padding alone; each misaligned pointer is refused."""
    import torch
    rules = cc.shadowed_tail(random_acl(41, 90, 0.2)[0], 2)
    r = len(rules) + 1
    tb = eng.put_table("device", rules)
    try:
        host = eng.table_cover(tb)
        pad = 64
        live = torch.full((r + 2 * pad,), 0x5A, dtype=torch.uint8, device="cuda")
        wit = torch.full((r + 2 * pad, 4), -7, dtype=torch.int32, device="cuda")
        cells = torch.full((r + 2 * pad,), -7, dtype=torch.int64, device="cuda")
        dead = torch.full((1 + 2 * pad,), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        out = (live[pad:pad + r], wit[pad:pad + r], cells[pad:pad + r], dead[pad:pad + 1])
        for mode in ("auto", "linear"):
            got = eng.table_cover(tb, mode=mode, out=out, stream=side)
            assert got["n_cells"] == host["n_cells"] and got["dims"] == host["dims"]
            side.synchronize()
            assert np.array_equal(out[0].cpu().numpy(), host["live"])
            assert out[1].cpu().numpy().tobytes() == host["witness"].tobytes()
            assert np.array_equal(out[2].cpu().numpy().view(np.uint64), host["cells"])
            assert int(out[3].item()) == host["n_dead"]
            for t, v in ((live, 0x5A), (wit, -7), (cells, -7), (dead, -7)):
                assert bool((t[:pad] == v).all()) and bool((t[-pad:] == v).all())
        # misaligned device pointers: refused with nothing written
        L = _abi.lib()
        n_cells, dims = np.full(1, 77, np.uint64), np.full(4, 77, np.uint32)
        ok = dict(live_out=live[pad:].data_ptr(), witness_out=wit[pad:].data_ptr(), cells_out=cells[pad:].data_ptr(),
                  n_dead=dead[pad:].data_ptr())
        before = [t.clone() for t in (live, wit, cells, dead)]
        for name, off in (("witness_out", 8), ("witness_out", 4), ("cells_out", 4), ("n_dead", 2)):
            p = dict(ok, **{name: ok[name] + off})
            o = _abi.CoverOut(p["live_out"], p["witness_out"], p["cells_out"], p["n_dead"], n_cells.ctypes.data,
                              dims.ctypes.data)
            assert L.cls_table_cover(eng.h, tb.id, 4, C.byref(o), _abi.F_DEVICE, None) == _abi.E_INVAL, name
            torch.cuda.synchronize()
            assert n_cells[0] == 77 and np.all(dims == 77)
            assert all(bool((a == b).all()) for a, b in zip(before, (live, wit, cells, dead))), name
    finally:
        eng.del_table(tb)


# ---- refusals ------------------------------------------------------------------

class _Raw:
    """Sentinel-filled host outputs of a raw cls_table_cover call."""

    def __init__(self, r):
        self.a = dict(live_out=np.zeros(r, np.uint8), witness_out=np.zeros(r, _abi.COVER_WITNESS),
                      cells_out=np.zeros(r, np.uint64), n_dead=np.zeros(1, np.uint32), n_cells=np.zeros(1, np.uint64),
                      dims=np.zeros(4, np.uint32))
        self.fill()

    def fill(self):
        for v in self.a.values():
            v.view(np.uint8)[:] = 0xA5

    def untouched(self):
        return all(bool((v.view(np.uint8) == 0xA5).all()) for v in self.a.values())

    def out(self, **kw):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        p.update(kw)
        return _abi.CoverOut(*[p[k] for k in ("live_out", "witness_out", "cells_out", "n_dead", "n_cells", "dims")])


def test_refusals_leave_the_outputs_alone(eng):
    from test_directed_traffic_cpu import refused_v16_table
    L = _abi.lib()
    rules = cc.shadowed_tail(random_acl(3, 30, 0.0)[0], 1)
    tb = eng.put_table("refusals", rules)
    raw = _Raw(len(rules) + 1)
    none = dict(live_out=None, witness_out=None, cells_out=None, n_dead=None)
    try:
        o = raw.out()
        for what, rc, args in (
                ("af 6", _abi.E_INVAL, (tb.id, 6, C.byref(o), 0)),
                ("af 0", _abi.E_INVAL, (tb.id, 0, C.byref(o), 0)),
                ("out NULL", _abi.E_INVAL, (tb.id, 4, None, 0)),
                ("no output", _abi.E_INVAL, (tb.id, 4, C.byref(raw.out(**none)), 0)),
                ("CLS_F_COUNT", _abi.E_INVAL, (tb.id, 4, C.byref(o), _abi.F_COUNT)),
                ("CLS_F_NO_VERDICT", _abi.E_INVAL, (tb.id, 4, C.byref(o), _abi.F_NO_VERDICT)),
                ("CLS_F_TIMING", _abi.E_INVAL, (tb.id, 4, C.byref(o), _abi.F_TIMING)),
                ("CLS_F_CONN_CLS", _abi.E_INVAL, (tb.id, 4, C.byref(o), _abi.F_CONN_CLS)),
                ("bit 31", _abi.E_INVAL, (tb.id, 4, C.byref(o), 1 << 31)),
                ("unknown table", _abi.E_NOTFOUND, (tb.id + 1000, 4, C.byref(o), 0))):
            assert L.cls_table_cover(eng.h, *args, None) == rc, what
            assert raw.untouched(), what
        # a V16 sweep of a table without a 16-byte classifier: cls_classify_rules' message
        t16 = eng.put_table("no16", refused_v16_table()[0])
        try:
            assert t16.info()["has_v16"] == 0
            assert L.cls_table_cover(eng.h, t16.id, 16, C.byref(o), 0, None) == _abi.E_INVAL
            assert b"no 16-byte classifier" in L.cls_last_error(eng.h) and raw.untouched()
        finally:
            eng.del_table(t16)
        # the next valid call is unharmed
        cc.assert_equal(eng.table_cover(tb), cc.cover_ref(rules), "after the refusals")
    finally:
        eng.del_table(tb)


def test_refusal_above_2_40_cells(eng):
    """4096 rules with distinct /32 sources and destinations and distinct
    single ports in a TCP and a UDP section: Ks = Kd = 8193, T = 16388, a
    product just above 2^40 (one rule fewer is below it).  The refusal
    precedes any device work, so nothing large runs."""
    L = _abi.lib()
    m = 4096
    assert (2 * m + 1) ** 2 * (4 * m + 4) > 1 << 40 > (2 * m - 1) ** 2 * (4 * m)
    ip = lambda x: "%d.%d.%d.%d/32" % (x >> 24, x >> 16 & 255, x >> 8 & 255, x & 255)
    rules = []
    for i in range(m):
        r = M.l4_rule(M.PERMIT, ip(0x0A000000 + 2 * i), ip(0x14000000 + 2 * i), "tcp", 0, 65535, 8 + 4 * i, 8 + 4 * i)
        r.matches.ip_rule.udp = M.Udp(destination_port_range=M.PortRange(9 + 4 * i, 9 + 4 * i),
                                      source_port_range=M.PortRange(0, 65535))
        rules.append(r)
    tb = eng.put_table("huge", rules)
    raw = _Raw(8)        # never written
    try:
        assert L.cls_table_cover(eng.h, tb.id, 4, C.byref(raw.out()), 0, None) == _abi.E_INVAL
        msg = L.cls_last_error(eng.h).decode()
        assert "Ks 8193" in msg and "Kd 8193" in msg and "T 16388" in msg, msg
        assert raw.untouched()
    finally:
        eng.del_table(tb)


# ---- ACLEngine.acl_coverage -----------------------------------------------------

def test_acl_coverage_on_a_rendered_scenario():
    """After every txn of one replayed renderer scenario: each installed ACL's
    dead rules, witnesses and default against the oracle over cells() of the
    rendered rules."""
    from scenario_replay import load_scenarios, replay
    from vpp_amd._abi import ClsError
    from vpp_amd.engine import ACLEngine, Engine
    test = [t for t in load_scenarios() if t["name"] == "TestCombinedRules"][0]
    seen = {"acls": 0, "live": 0}

    def dotted(a):
        return "%d.%d.%d.%d" % (a >> 24, a >> 16 & 255, a >> 8 & 255, a & 255)

    def check(engine, calls):
        for name, acl in engine.by_name.items():
            ref = cc.cover_ref(acl.rules)
            got = engine.acl_coverage(name)
            r = len(acl.rules)
            assert got["dead"] == [k for k in range(r) if not ref["live"][k]], name
            assert got["default_reachable"] == bool(ref["live"][r]), name
            w = ref["witness"]
            assert got["witness"] == {k: (dotted(int(w[k]["src"])), dotted(int(w[k]["dst"])), int(w[k]["proto"]),
                                          int(w[k]["dport"])) for k in range(r) if ref["live"][k]}, name
            assert engine.acl_coverage(name, af=16) == got, name
            seen["acls"] += 1
            seen["live"] += len(got["witness"])
        with pytest.raises(ClsError):
            engine.acl_coverage("no such acl")
        return engine.connection_batch(calls)

    _, failures = replay(test, lambda contiv: ACLEngine(contiv, Engine()), check_conn=check)
    assert not failures, "\n".join(failures)
    assert seen["acls"] >= 2 and seen["live"] >= 2


# ---- Go shims -------------------------------------------------------------------

@pytest.mark.parametrize("fam", [4, 16])
def test_go_shims_table_cover(fam, tmp_path, eng):
    """go/shimtest/tablecover (gcc): the sweep through clsg_table_cover_v4 /
    clsg_table_cover_v16, as the Go binding's TableCover calls them; its output
    files equal the reference."""
    from test_gpu_reach import _write_acls
    if not os.path.exists(TABLECOVER):
        subprocess.run(["make", "-s", "-C", os.path.dirname(TABLECOVER)], check=True)
    rules = cc.shadowed_tail((random_acl16 if fam == 16 else random_acl)(19, 60, 0.2)[0], 6)
    ref = cc.cover_ref(rules, fam)
    _write_acls(tmp_path / "acls.txt", {"by_name": {"cover": rules}, "ifs": ["if0"], "bind": {"if0": ("cover", None)}})
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(
        [os.path.join(ROOT, "vpp_amd")] + [x for x in [os.environ.get("LD_LIBRARY_PATH")] if x]))
    r = subprocess.run([TABLECOVER, str(tmp_path), str(fam)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.fromfile(tmp_path / "out_cover_live.bin", np.uint8), ref["live"])
    assert (tmp_path / "out_cover_witness.bin").read_bytes() == ref["witness"].tobytes()
    assert np.array_equal(np.fromfile(tmp_path / "out_cover_cells.bin", "<u8"), ref["cells"])
    assert int(np.fromfile(tmp_path / "out_cover_dead.bin", "<u4")[0]) == ref["n_dead"]
    assert int(np.fromfile(tmp_path / "out_cover_n.bin", "<u8")[0]) == ref["n_cells"]
    assert tuple(np.fromfile(tmp_path / "out_cover_dims.bin", "<u4")) == tuple(ref["dims"])
