"""GPU tests of the rule necessity sweep (cls_table_need, Engine.table_need,
ACLEngine.acl_needed / acl_minimize, the Go shim).

Bar: bit-exact equality with need_cases.need_ref -- the OpenMP oracle over the
representative packet of every cell, and over the list without r on r's cells
-- whose shortcut test_table_need_cpu.py pins to the literal definition; and
agreement with what exists: cls_table_cover's counts, cls_table_diff of the
list against the list without a rule.  Every table stays below 2^16 cells."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cover_cases as cc
import need_cases as nc
from test_table_need_cpu import SIZES, random_table
from vpp_amd import _abi
from vpp_amd import model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLENEED = os.path.join(ROOT, "go", "shimtest", "tableneed")
NAMES = ("need", "free", "first", "changed", "witness", "counts")


@pytest.fixture(scope="module")
def eng():
    from vpp_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _need(eng, rules, skip=None, want=None, what=""):
    t = eng.put_table("need", rules)
    try:
        got = eng.table_need(t, skip=skip)
    finally:
        eng.del_table(t)
    if want is not None:
        nc.assert_equal(got, want, what)
    return got


# ---- 1. the constructed ACLs ----------------------------------------------------

def test_constructed_need_acl(eng):
    rules = nc.need_acl()
    at = nc.names(rules).index
    got = _need(eng, rules, want=nc.ref("need_acl", rules), what="need_acl")
    need, free, w = got["need"], got["free"], got["witness"]
    assert need[at("deny_udp")] == nc.REDUNDANT and free[at("deny_udp")] == 1
    assert need[at("a32")] == nc.REDUNDANT and w[at("a32")]["after"] == 0
    assert need[at("b32")] == nc.NEEDED
    assert tuple(w[at("b32")]) == (10 << 24 | 1 << 16 | 5, 0, 80, 0, 0x80, at("bdeny"))
    assert need[at("c24")] == nc.DEAD
    assert (need[at("d1")], free[at("d1")], need[at("d2")], free[at("d2")]) == (nc.REDUNDANT, 0, nc.DEAD, 1)
    assert need[at("e1")] == nc.NEEDED and w[at("e1")]["after"] == 0x82
    assert need[at("f1")] == nc.NEEDED and w[at("f1")]["after"] == 0x81
    assert need[at("g")] == nc.NEEDED and w[at("g")]["proto"] == 3
    # after one round d1 becomes NEEDED
    gone = [k for k in range(len(rules)) if free[k]]
    again = _need(eng, rules, skip=gone, want=nc.ref("need_acl", rules, gone), what="need_acl, second round")
    assert again["need"][at("d1")] == nc.NEEDED


def test_constructed_unconditional_failure(eng):
    rules = nc.need_acl_fail()
    got = _need(eng, rules, want=nc.ref("need_acl_fail", rules), what="need_acl_fail")
    assert got["need"].tolist() == [nc.NEEDED, nc.NEEDED, nc.DEAD, nc.DEAD]
    assert got["witness"][1]["fall"] == 2


# ---- 2. random lists at the word edges ------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_random_parity(eng, n):
    rules = random_table(n)
    _need(eng, rules, want=nc.ref("random%d" % n, rules), what="random %d" % n)


# ---- 3, 4. more than one word per lane; more rules than the fold's LDS bins --------

@pytest.mark.parametrize("lds", [1, 0])
def test_second_word_per_lane(eng, lds):
    """R = 4,200, W = 66: first and second matches across words 0, 63 and 64."""
    rules = nc.strided_acl()
    eng.set_option("need_cols_lds", lds)
    try:
        got = _need(eng, rules, want=nc.ref("strided", rules), what="strided lds %d" % lds)
    finally:
        eng.set_option("need_cols_lds", None)
    assert got["witness"][0]["fall"] == 1 and got["witness"][2]["fall"] == 4100
    assert got["need"][4040] == nc.REDUNDANT and got["free"][4040] == 0 and got["need"][4110] == nc.DEAD


@pytest.mark.parametrize("n", [15400, 16450])
def test_more_rules_than_the_folds_lds_bins(eng, n):
    """15,400 rules: the sentinel fold's n_out = R + 2 is above cover_fold's
    15,360 LDS bins.  16,450 rules: W = 258, above the 256 words need_cells
    keeps in registers (the form that reads every row per cell)."""
    rules = nc.many_rules_acl(n)
    assert n + 2 > 15360 and cc.dims(rules)[1] < nc.MAX_CELLS
    want = nc.ref("many%d" % n, rules)
    assert want["need"][n - 3] == nc.REDUNDANT and want["need"][n - 2] == nc.NEEDED and want["need"][n - 1] == nc.DEAD
    for tile in (1024, None):
        eng.set_option("cover_tile", tile)
        try:
            _need(eng, rules, want=want, what="%d rules, tile %s" % (n, tile))
        finally:
            eng.set_option("cover_tile", None)


# ---- 5, 6. tiling and the two column forms -----------------------------------------

def _wide_table():
    """262 rules with T = 528 columns above half of the smallest cover_tile, 12
    (s, d) pairs: tiles of one pair (1024), of 7 and a ragged 5 (4096), one tile."""
    rules = []
    for i in range(260):
        rules.append(nc._l4("p%d" % i, "10.%d.0.0/16" % (i % 2), "tcp", 4 * i, 4 * i + 1 + i % 2,
                            M.DENY if i % 3 == 0 else M.PERMIT, dst="" if i % 5 else "10.9.0.0/16"))
    rules.append(nc._l4("dup", "10.1.0.0/16", "tcp", 28, 30))           # p7 again: dead
    rules.append(nc._l4("again", "10.1.0.0/16", "tcp", 0, 700))
    rules.append(nc._l4("deny_tcp", "", "tcp", 0, 65535, M.DENY))
    return rules


def test_tiling_and_column_forms(eng):
    rules = _wide_table()
    (ks, kd, kt, ku), n_cells = cc.dims(rules)
    t = kt + ku + 2
    assert 512 < t and 4096 // t == 7 and ks * kd == 12 and n_cells < nc.MAX_CELLS
    want = nc.ref("wide", rules)
    assert all(want["counts"][v] > 0 for v in (nc.DEAD, nc.REDUNDANT, nc.NEEDED))
    tb = eng.put_table("wide", rules)
    try:
        for lds in (1, 0):
            for tile in (1024, 4096, None):
                eng.set_option("cover_tile", tile)
                eng.set_option("need_cols_lds", lds)
                nc.assert_equal(eng.table_need(tb), want, "tile %s lds %d" % (tile, lds))
    finally:
        eng.set_option("cover_tile", None)
        eng.set_option("need_cols_lds", None)
        eng.del_table(tb)


@pytest.mark.parametrize("table", ["need_acl", "random130"])
def test_columns_from_global_memory(eng, table):
    rules = nc.need_acl() if table == "need_acl" else random_table(130)
    eng.set_option("need_cols_lds", 0)
    try:
        _need(eng, rules, want=nc.ref(table, rules), what=table + " lds 0")
    finally:
        eng.set_option("need_cols_lds", None)


# ---- 7. skip ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 130])
def test_skip(eng, n):
    rules = random_table(n)
    tb = eng.put_table("skip", rules)
    try:
        for r in (0, n // 2, 63, 64, n - 1):
            got = eng.table_need(tb, skip=[r])
            nc.assert_equal(got, nc.ref("random%d" % n, rules, [r]), "skip %d" % r)
            short = _need(eng, rules[:r] + rules[r + 1:])
            keep = np.arange(n) != r
            assert np.array_equal(got["need"][keep], short["need"]) and np.array_equal(got["free"][keep], short["free"])
            w = short["witness"].copy()
            w["fall"][(w["after"] != 0) & (w["fall"] >= r)] += 1
            assert got["witness"][keep].tobytes() == w.tobytes()
        got = eng.table_need(tb, skip=range(n))
        assert np.all(got["need"] == nc.SKIPPED) and got["first"][n] == got["n_cells"]
        assert got["counts"].tolist() == [n, 0, 0, 0] and not got["free"].any() and not got["changed"].any()
        assert got["witness"].tobytes() == bytes(16 * n)
    finally:
        eng.del_table(tb)


# ---- 8. the device form and the refusals -----------------------------------------------

def test_device_form(eng):
    """torch outputs inside 64 padding elements on a side stream equal the
    host form and leave the padding alone; each misaligned pointer is refused."""
    import torch
    rules = random_table(130)
    r = len(rules)
    tb = eng.put_table("device", rules)
    try:
        host = eng.table_need(tb, skip=[7])
        pad = 64
        full = [torch.full((r + 2 * pad,), 0x5A, dtype=torch.uint8, device="cuda"),
                torch.full((r + 2 * pad,), 0x5A, dtype=torch.uint8, device="cuda"),
                torch.full((r + 1 + 2 * pad,), -7, dtype=torch.int64, device="cuda"),
                torch.full((r + 2 * pad,), -7, dtype=torch.int64, device="cuda"),
                torch.full((r + 2 * pad, 4), -7, dtype=torch.int32, device="cuda"),
                torch.full((4 + 2 * pad,), -7, dtype=torch.int32, device="cuda")]
        lens = (r, r, r + 1, r, r, 4)
        out = tuple(t[pad:pad + n] for t, n in zip(full, lens))
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        got = eng.table_need(tb, skip=[7], out=out, stream=side)
        assert got["n_cells"] == host["n_cells"] and got["dims"] == host["dims"]
        side.synchronize()
        for name, o in zip(NAMES, out):
            assert o.cpu().numpy().tobytes() == host[name].tobytes(), name
        for t, v in zip(full, (0x5A, 0x5A, -7, -7, -7, -7)):
            assert bool((t[:pad] == v).all()) and bool((t[-pad:] == v).all())
        # without free_out (no second pass) the other outputs are the same
        for t, v in zip(full, (0x5A, 0x5A, -7, -7, -7, -7)):
            t.fill_(v)
        torch.cuda.synchronize()
        eng.table_need(tb, skip=[7], out=(out[0], False) + out[2:], stream=side)
        side.synchronize()
        for name, o in zip(NAMES, out):
            if name != "free":
                assert o.cpu().numpy().tobytes() == host[name].tobytes(), name
        assert bool((full[1] == 0x5A).all())
        # misaligned device pointers: refused with nothing written
        L = _abi.lib()
        n_cells, dims = np.full(1, 77, np.uint64), np.full(4, 77, np.uint32)
        ok = [t[pad:].data_ptr() for t in full]
        before = [t.clone() for t in full]
        for i, off in ((4, 8), (4, 4), (2, 4), (3, 4), (5, 2)):
            p = list(ok)
            p[i] += off
            o = _abi.NeedOut(*p, n_cells.ctypes.data, dims.ctypes.data)
            assert L.cls_table_need(eng.h, tb.id, None, C.byref(o), _abi.F_DEVICE, None) == _abi.E_INVAL, (i, off)
            torch.cuda.synchronize()
            assert n_cells[0] == 77 and np.all(dims == 77)
            assert all(bool((a == b).all()) for a, b in zip(before, full)), (i, off)
    finally:
        eng.del_table(tb)


class _Raw:
    """Canary-filled host outputs of a raw cls_table_need call."""
    FIELDS = ("need_out", "free_out", "first_out", "changed_out", "witness_out", "counts", "n_cells", "dims")

    def __init__(self, r):
        self.a = dict(need_out=np.zeros(r, np.uint8), free_out=np.zeros(r, np.uint8), first_out=np.zeros(r + 1, np.uint64),
                      changed_out=np.zeros(r, np.uint64), witness_out=np.zeros(r, _abi.NEED_WITNESS),
                      counts=np.zeros(4, np.uint32), n_cells=np.zeros(1, np.uint64), dims=np.zeros(4, np.uint32))
        for v in self.a.values():
            v.view(np.uint8)[:] = 0xA5

    def untouched(self):
        return all(bool((v.view(np.uint8) == 0xA5).all()) for v in self.a.values())

    def out(self, **kw):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        p.update(kw)
        return _abi.NeedOut(*[p[k] for k in self.FIELDS])


def test_refusals_leave_the_outputs_alone(eng):
    L = _abi.lib()
    rules = random_table(63)
    tb = eng.put_table("refusals", rules)
    raw = _Raw(len(rules))
    none = {k: None for k in _Raw.FIELDS[:6]}
    try:
        o = raw.out()
        for what, rc, args in (
                ("out NULL", _abi.E_INVAL, (tb.id, None, None, 0)),
                ("no output", _abi.E_INVAL, (tb.id, None, C.byref(raw.out(**none)), 0)),
                ("CLS_F_FORCE_LINEAR", _abi.E_INVAL, (tb.id, None, C.byref(o), _abi.F_FORCE_LINEAR)),
                ("CLS_F_COUNT", _abi.E_INVAL, (tb.id, None, C.byref(o), _abi.F_COUNT)),
                ("CLS_F_NO_VERDICT | CLS_F_DEVICE", _abi.E_INVAL, (tb.id, None, C.byref(o), _abi.F_NO_VERDICT | 1)),
                ("bit 31", _abi.E_INVAL, (tb.id, None, C.byref(o), 1 << 31)),
                ("unknown table", _abi.E_NOTFOUND, (tb.id + 1000, None, C.byref(o), 0))):
            assert L.cls_table_need(eng.h, *args, None) == rc, what
            assert raw.untouched(), what
        # the bit rows above the cap: the numbers are in the message
        eng.set_option("need_bitmap_mb", 0)
        try:
            assert L.cls_table_need(eng.h, tb.id, None, C.byref(o), 0, None) == _abi.E_INVAL
            msg = L.cls_last_error(eng.h).decode()
            ks, kd, kt, ku = cc.dims(rules)[0]
            assert "need_bitmap_mb 0" in msg and "Ks %d" % ks in msg and "T %d" % (kt + ku + 2) in msg, msg
            assert raw.untouched()
        finally:
            eng.set_option("need_bitmap_mb", None)
        with pytest.raises(_abi.ClsError):
            eng.set_option("need_bitmap_mb", -1)
        # the next valid call is unharmed
        nc.assert_equal(eng.table_need(tb), nc.ref("random63", rules), "after the refusals")
    finally:
        eng.del_table(tb)


def test_refusal_above_2_40_cells(eng):
    """test_gpu_table_cover's list just above 2^40 cells: refused before any device work."""
    L = _abi.lib()
    m = 4096
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
        assert L.cls_table_need(eng.h, tb.id, None, C.byref(raw.out()), 0, None) == _abi.E_INVAL
        msg = L.cls_last_error(eng.h).decode()
        assert "Ks 8193" in msg and "Kd 8193" in msg and "T 16388" in msg, msg
        assert raw.untouched()
    finally:
        eng.del_table(tb)


# ---- 9. ties to what exists ---------------------------------------------------------------

TIE_TABLES = {"need_acl": nc.need_acl, "need_acl_fail": nc.need_acl_fail, "random130": lambda: random_table(130),
              "random65": lambda: random_table(65)}


@pytest.mark.parametrize("table", sorted(TIE_TABLES))
def test_ties_to_cover_and_diff(eng, table):
    rules = TIE_TABLES[table]()
    n = len(rules)
    ta = eng.put_table("tie", rules)
    try:
        got = eng.table_need(ta)
        for af in (4, 16):
            cov = eng.table_cover(ta, af=af)
            assert np.array_equal(got["first"], cov["cells"]), af
            assert np.array_equal(got["need"] == nc.DEAD, cov["live"][:n] == 0), af
        rng = np.random.default_rng(len(table))
        some = sorted(set(rng.choice(n, min(16, n), replace=False).tolist()) |
                      set(np.flatnonzero(got["need"] == nc.NEEDED)[:4].tolist()))
        act = {}
        for r in some:
            tb = eng.put_table("tie without", rules[:r] + rules[r + 1:])
            try:
                d = eng.table_diff(ta, tb, rec_cap=1)
            finally:
                eng.del_table(tb)
            assert d["equal"] == (got["need"][r] != nc.NEEDED), r
            if not d["equal"]:
                rec, w = d["records"][0], got["witness"][r]
                assert (rec["src_lo"], rec["dst_lo"], rec["proto"], rec["port_lo"]) == \
                    (w["src"], w["dst"], w["proto"], w["dport"]), r
                assert rec["rule_a"] == r and rec["now"] == w["after"] & 3 and w["after"] & 0x80
                assert rec["rule_b"] + (1 if rec["rule_b"] >= r else 0) == w["fall"], r
                f = d["first"]
                assert (f["src"], f["dst"], f["proto"], f["dport"]) == (w["src"], w["dst"], w["proto"], w["dport"])
                act[r] = int(rec["was"])
        assert act or not (got["need"] == nc.NEEDED).any()
        # deleting ALL free rules at once changes no verdict
        keep = [k for k in range(n) if not got["free"][k]]
        assert len(keep) < n
        tb = eng.put_table("tie free", [rules[k] for k in keep])
        try:
            assert eng.table_diff(ta, tb, rec_cap=0)["equal"]
        finally:
            eng.del_table(tb)
    finally:
        eng.del_table(ta)


def test_acl_needed_and_minimize():
    from vpp_amd._abi import ClsError
    from vpp_amd.engine import ACLEngine, Engine
    rules = nc.need_acl()
    at = nc.names(rules).index
    want = nc.ref("need_acl", rules)
    ae = ACLEngine(None, Engine())
    try:
        acl = M.Acl(rules=rules, acl_name="a", interfaces=M.Interfaces(ingress=["if0"]))
        assert ae.apply_txn([(M.acl_key("a"), acl)]) is None
        got = ae.acl_needed("a")
        n = len(rules)
        assert got["dead"] == np.flatnonzero(want["need"] == nc.DEAD).tolist()
        assert got["redundant"] == np.flatnonzero(want["need"] == nc.REDUNDANT).tolist()
        assert got["free"] == np.flatnonzero(want["free"]).tolist()
        assert sorted(got["needed"]) == np.flatnonzero(want["need"] == nc.NEEDED).tolist()
        assert got["needed"][at("b32")] == ("10.1.0.5", "0.0.0.0", 0, 80, 0, at("bdeny"))
        assert got["needed"][at("e1")][4:] == (2, at("e2"))
        assert got["default_reachable"] == bool(want["first"][n])
        assert at("d2") not in ae.acl_needed("a", keep=[at("d2")])["free"]
        with pytest.raises(ClsError):
            ae.acl_needed("no such acl")
        with pytest.raises(ClsError):
            ae.acl_minimize("no such acl")
        # the rule with an IPv6 network survives by default
        kept, rounds = ae.acl_minimize("a")
        assert len(rounds) == 2 and at("v6") in kept and at("d1") in kept and at("deny_tcp") in rounds[1]
        removed = [k for r in rounds for k in r]
        assert sorted(kept + removed) == list(range(n))
        ta = ae.engine.acl_table("a")
        tb = ae.engine.put_table("minimized", [rules[k] for k in kept])
        try:
            assert ae.engine.table_diff(ta, tb, rec_cap=0)["equal"]
            own = ae.engine.table_need(tb)
            loose = [kept[i] for i in np.flatnonzero((own["need"] == nc.DEAD) | (own["need"] == nc.REDUNDANT))]
            assert loose == [at("v6")]
        finally:
            ae.engine.del_table(tb)
        kept6, rounds6 = ae.acl_minimize("a", keep_v6=False)
        assert at("v6") in rounds6[0] and at("v6") not in kept6
        assert ae.acl_minimize("a", keep=[at("d2")])[0].count(at("d2")) == 1
        assert ae.get_num_of_acls() == 1                      # nothing was installed
    finally:
        ae.engine.close()


# ---- the Go shim ---------------------------------------------------------------------------

@pytest.mark.parametrize("skip", [None, 3])
def test_go_shim_table_need(skip, tmp_path):
    """go/shimtest/tableneed (gcc): the sweep through clsg_table_need, as the
    Go binding's TableNeed calls it; its output files equal the reference."""
    from test_gpu_reach import _write_acls
    if not os.path.exists(TABLENEED):
        subprocess.run(["make", "-s", "-C", os.path.dirname(TABLENEED)], check=True)
    rules = random_table(65)
    want = nc.ref("random65", rules, [] if skip is None else [skip])
    _write_acls(tmp_path / "acls.txt", {"by_name": {"need": rules}, "ifs": ["if0"], "bind": {"if0": ("need", None)}})
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(
        [os.path.join(ROOT, "vpp_amd")] + [x for x in [os.environ.get("LD_LIBRARY_PATH")] if x]))
    r = subprocess.run([TABLENEED, str(tmp_path)] + ([] if skip is None else [str(skip)]), capture_output=True,
                       text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.fromfile(tmp_path / "out_need_need.bin", np.uint8), want["need"])
    assert np.array_equal(np.fromfile(tmp_path / "out_need_free.bin", np.uint8), want["free"])
    assert np.array_equal(np.fromfile(tmp_path / "out_need_first.bin", "<u8"), want["first"])
    assert np.array_equal(np.fromfile(tmp_path / "out_need_changed.bin", "<u8"), want["changed"])
    assert (tmp_path / "out_need_witness.bin").read_bytes() == want["witness"].tobytes()
    assert np.array_equal(np.fromfile(tmp_path / "out_need_counts.bin", "<u4"), want["counts"])
    assert int(np.fromfile(tmp_path / "out_need_n.bin", "<u8")[0]) == want["n_cells"]
    assert tuple(np.fromfile(tmp_path / "out_need_dims.bin", "<u4")) == tuple(want["dims"])
