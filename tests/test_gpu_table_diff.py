"""GPU tests of the table diff (cls_table_diff, Engine.table_diff,
ACLEngine.acl_diff, the Go shims).

Bar: bit-exact equality with table_diff_cases.diff_ref -- the OpenMP oracle
under both rule lists over the representative packets of every joint cell,
reduced with numpy -- whose own soundness test_table_diff_cpu.py states without
classes.  Every pair of lists stays at or below 2^22 joint cells."""
import copy
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cover_cases as cc
import table_diff_cases as td
from aclgen import random_acl, random_acl16, single_port_acl
from vpp_amd import _abi
from vpp_amd import model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLEDIFF = os.path.join(ROOT, "go", "shimtest", "tablediff")


@pytest.fixture(scope="module")
def eng():
    from vpp_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _diff(eng, a, b, af=4, mode="auto", want=None, what="", **kw):
    ta, tb = eng.put_table("diff a", a), eng.put_table("diff b", b)
    try:
        got = eng.table_diff(ta, tb, af=af, mode=mode, **kw)
    finally:
        eng.del_table(ta)
        eng.del_table(tb)
    if want is not None:
        td.assert_equal(got, want, what)
    return got


def _all_rules(action, src=""):
    """Three rules that together take every packet from src with the action:
    every TCP port (and, by its networks alone, every protocol above 2), every
    UDP port, ICMP."""
    return [cc._l4("all tcp", src, "tcp", 0, 65535, action), cc._l4("all udp", src, "udp", 0, 65535, action),
            M.icmp_rule(action, src)]


# ---- random parity ------------------------------------------------------------

# lists whose first seed has no live PERMIT / DENY rule (an early rule fails every packet) take a later one
_LATER = {(4, 5, 0.3): 1, (16, 5, 0.3): 1, (16, 80, 0.3): 2, (16, 400, 0.3): 4}
_SIZES, _WEIRD, _AFS = (5, 80, 400), (0.0, 0.3), (4, 16)


@functools.lru_cache(maxsize=None)
def _parity_case(n, weird, af):
    seed = n * 3 + int(weird * 10) + 1 + 1000 * _LATER.get((af, n, weird), 0)
    a = cc.shadowed_tail((random_acl16 if af == 16 else random_acl)(seed, n, weird)[0], n)
    b = td.edit(a, af)
    return a, b, td.diff_ref(a, b, af)


@pytest.mark.parametrize("mode", ["auto", "linear"])
@pytest.mark.parametrize("af", _AFS)
@pytest.mark.parametrize("weird", _WEIRD)
@pytest.mark.parametrize("n", _SIZES)
def test_random_parity(eng, n, weird, af, mode):
    a, b, ref = _parity_case(n, weird, af)
    assert 1 <= ref["n_diff"] < ref["n_cells"] and ref["n_rec"] >= 2          # no vacuous pass
    _diff(eng, a, b, af, mode, want=ref, what="random %d %.1f af %d %s" % (n, weird, af, mode))


def test_random_parity_sees_several_transitions():
    seen = set()
    for n in _SIZES:
        for weird in _WEIRD:
            for af in _AFS:
                p = _parity_case(n, weird, af)[2]["pairs"]
                seen |= {(i, j) for i in range(4) for j in range(4) if i != j and p[i, j]}
    assert len(seen) >= 2, seen


@pytest.mark.parametrize("af", _AFS)
def test_independent_lists(eng, af):
    gen = random_acl16 if af == 16 else random_acl
    a, b = gen(1201, 400, 0.0)[0], gen(1202, 400, 0.0)[0]
    ref = td.diff_ref(a, b, af)
    assert 1 << 20 < ref["n_cells"] <= cc.MAX_CELLS and ref["n_rec"] > 10000
    _diff(eng, a, b, af, want=ref, what="independent af %d" % af)


# ---- equivalence ----------------------------------------------------------------

def _assert_no_difference(got):
    assert got["equal"] and got["n_diff"] == 0 and got["n_rec"] == 0 and len(got["records"]) == 0
    assert np.array_equal(got["pairs"], np.diag(np.diag(got["pairs"]))) and int(got["pairs"].sum()) == got["n_cells"]
    assert got["first"].tobytes() == bytes(16)
    for k in ("cells_a", "cells_b", "wit_a", "wit_b"):
        assert got[k].tobytes() == bytes(got[k].nbytes), k


@pytest.mark.parametrize("af", _AFS)
def test_equivalent_lists(eng, af):
    a = cc.shadowed_tail(random_acl(16, 60, 0.0)[0], 5)
    e, done = td.equivalent(a)
    assert all(done.values())
    ref = td.diff_ref(a, e, af)
    assert ref["equal"] and tuple(ref["dims"]) != cc.dims(a)[0]
    _assert_no_difference(_diff(eng, a, e, af, want=ref, what="equivalent"))
    # a table against itself, and against a re-put of its rules
    t = eng.put_table("self", a)
    t2 = eng.put_table("again", copy.deepcopy(a))
    try:
        for other in (t, t2):
            got = eng.table_diff(t, other, af=af)
            _assert_no_difference(got)
            td.assert_equal(got, td.diff_ref(a, a, af), "self")
    finally:
        eng.del_table(t)
        eng.del_table(t2)


# ---- independence of the evaluator and the tile -----------------------------------

def _row_pair():
    """An 80-rule list and its edit, each behind rules for every packet from
    10.0.0.0/8 -- DENY in a, PERMIT in b: every cell of those rows differs, so
    a run ends on each row's last column while the next row's first differs."""
    a, b, _ = _parity_case(80, 0.0, 4)
    return _all_rules(M.DENY, "10.0.0.0/8") + a, _all_rules(M.PERMIT, "10.0.0.0/8") + b


def _port_pair():
    """600 port rules behind a rule for every TCP port -- DENY in a, PERMIT in
    b, where one UDP rule's action is flipped and another deleted as well: Ks =
    Kd = 1 and T above 1024, a one-row tile above cover_tile 1024, and the TCP
    columns one run longer than the 256 cells a wave holds."""
    a = [cc._l4("p%d" % i, "", "tcp" if i % 2 else "udp", 100 * i, 100 * i + 49) for i in range(1, 601)]
    b = [copy.deepcopy(r) for r in a]
    b[11].actions.acl_action = M.DENY
    del b[21]
    return [cc._l4("tcp", "", "tcp", 0, 65535, M.DENY)] + a, [cc._l4("tcp", "", "tcp", 0, 65535, M.PERMIT)] + b


def _check_row_pair(ref):
    (ks, kd, kt, ku), n = ref["dims"], ref["n_cells"]
    t = kt + ku + 2
    assert t & (t - 1) and 1024 % t and 2048 % t and n > 4096
    m = ref["mask"]
    ends = np.flatnonzero(m[t - 1:n - 1:t] & m[t::t])           # rows whose last cell and successor differ
    assert len(ends) >= 2
    whole = m.reshape(-1, t).all(1)                             # rows every cell of which differs
    assert np.any(whole[:-1] & whole[1:])
    # ... which are two records, one per row: the reference cuts a run at every row and protocol
    assert int((ref["records"]["proto"] == 3).sum()) >= len(ends)


@pytest.mark.parametrize("af", _AFS)
@pytest.mark.parametrize("opts", [{}, {"orient": "src"}, {"orient": "dst"}, {"list_mode": "0"}, {"list_mode": "1"},
                                  {"list_mode": "3"}, {"orient": "src", "trie": "1", "wide": "0"},
                                  {"orient": "src", "trie": "1", "wide": "1"},
                                  {"orient": "src", "trie": "0", "wide": "1"}],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "default")
def test_evaluator_and_tile_independence(eng, libopt, opts, af):
    """The result is the same whichever image the compiler is forced to build
    and however many rows a tile holds."""
    a, b = _row_pair()
    ref = td.diff_ref(a, b, af)
    _check_row_pair(ref)
    for k, v in opts.items():
        libopt.set(k, v, eng)
    ta, tb = eng.put_table("ind a", a), eng.put_table("ind b", b)
    try:
        for tile in (1024, 2048, (ref["n_cells"] + 1023) & ~1023, None):
            eng.set_option("cover_tile", tile)
            td.assert_equal(eng.table_diff(ta, tb, af=af), ref, "%s tile %s af %d" % (opts, tile, af))
    finally:
        eng.set_option("cover_tile", None)
        eng.del_table(ta)
        eng.del_table(tb)


@pytest.mark.parametrize("af", _AFS)
def test_one_row_tile_above_cover_tile(eng, af):
    a, b = _port_pair()
    ref = td.diff_ref(a, b, af)
    assert ref["dims"][:2] == (1, 1) and ref["dims"][2] + ref["dims"][3] + 2 > 1024 and ref["n_rec"] >= 3
    # the TCP columns are one run; the front rule also takes the protocols above 2
    assert ref["dims"][2] > 256 and int(ref["cells_a"][0]) == ref["dims"][2] + 1
    assert tuple(ref["records"][0])[4:7] == (0, 65535, 0)
    for tile in (1024, None):
        eng.set_option("cover_tile", tile)
        try:
            for mode in ("auto", "linear"):
                _diff(eng, a, b, af, mode, want=ref, what="T > 1024, tile %s %s" % (tile, mode))
        finally:
            eng.set_option("cover_tile", None)


def test_single_port_trie_lists(eng, libopt):
    a = cc.shadowed_tail(single_port_acl(22, 300, n_prefixes=24)[0], 3)
    b = td.edit(a)
    ref = td.diff_ref(a, b)
    assert ref["n_diff"] >= 1
    libopt.set("orient", "src", eng)
    libopt.set("trie", "1", eng)
    libopt.set("wide", "1", eng)
    _diff(eng, a, b, want=ref, what="single-port lists")


def test_v4_and_v16_diffs_agree(eng):
    a, b, ref = _parity_case(80, 0.0, 4)
    g4, g16 = _diff(eng, a, b, 4), _diff(eng, a, b, 16)
    td.assert_equal(g16, g4, "v16 against v4")
    td.assert_equal(g4, ref, "v4")


# ---- the record cap -------------------------------------------------------------

class _Raw:
    """Sentinel-filled host outputs of a raw cls_table_diff call."""
    ORDER = ("n_diff", "pairs_out", "first_out", "cells_a", "wit_a", "cells_b", "wit_b", "rec_out", "rec_cap",
             "n_rec", "n_cells", "dims")

    def __init__(self, ra, rb, recs):
        w = _abi.COVER_WITNESS
        self.a = dict(n_diff=np.zeros(1, np.uint64), pairs_out=np.zeros(16, np.uint64), first_out=np.zeros(1, w),
                      cells_a=np.zeros(ra, np.uint64), wit_a=np.zeros(ra, w), cells_b=np.zeros(rb, np.uint64),
                      wit_b=np.zeros(rb, w), rec_out=np.zeros(max(1, recs), _abi.TDIFF_REC),
                      n_rec=np.zeros(1, np.uint64), n_cells=np.zeros(1, np.uint64), dims=np.zeros(4, np.uint32))
        self.fill()

    def fill(self):
        for v in self.a.values():
            v.view(np.uint8)[:] = 0xA5

    def untouched(self):
        return all(bool((v.view(np.uint8) == 0xA5).all()) for v in self.a.values())

    def out(self, rec_cap=0, **kw):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        p["rec_cap"] = rec_cap
        p.update(kw)
        return _abi.TDiffOut(*[p[k] for k in self.ORDER])


def test_record_cap(eng):
    a, b, ref = _parity_case(80, 0.0, 4)
    n = ref["n_rec"]
    L = _abi.lib()
    ta, tb = eng.put_table("cap a", a), eng.put_table("cap b", b)
    try:
        for cap in (0, 1, n - 1, n, n + 7):
            raw = _Raw(len(a) + 1, len(b) + 1, n + 16)
            o = raw.out(rec_cap=cap, rec_out=raw.a["rec_out"].ctypes.data if cap else None)
            assert L.cls_table_diff(eng.h, ta.id, tb.id, 4, C.byref(o), 0, None) == 0, cap
            keep = min(cap, n)
            assert int(raw.a["n_rec"][0]) == n and int(raw.a["n_diff"][0]) == ref["n_diff"], cap
            assert raw.a["rec_out"][:keep].tobytes() == ref["records"][:keep].tobytes(), cap
            assert bool((raw.a["rec_out"][keep:].view(np.uint8) == 0xA5).all()), cap
            td.assert_equal(eng.table_diff(ta, tb, rec_cap=cap), ref, "cap %d" % cap, rec_cap=cap)
    finally:
        eng.del_table(ta)
        eng.del_table(tb)


# ---- degenerate shapes --------------------------------------------------------

@pytest.mark.parametrize("af", _AFS)
def test_degenerate_shapes(eng, af):
    got = _diff(eng, [], [], af, want=td.diff_ref([], [], af), what="[] against []")
    _assert_no_difference(got)
    assert got["dims"] == (1, 1, 1, 1) and got["n_cells"] == 4 and int(got["pairs"][0, 0]) == 4
    # [] against allow-all: every cell 0 -> 1, one record per row and protocol
    allow = _all_rules(M.PERMIT)
    ref = td.diff_ref([], allow, af)
    got = _diff(eng, [], allow, af, want=ref, what="[] against allow-all")
    assert got["n_diff"] == got["n_cells"] == 4 and int(got["pairs"][0, 1]) == 4 and got["n_rec"] == 4
    assert got["records"]["proto"].tolist() == [0, 1, 2, 3] and np.all(got["records"]["port_hi"] == 65535)
    assert np.all(got["records"]["src_hi"] == 0xFFFFFFFF) and got["cells_a"].tolist() == [4]
    assert got["cells_b"].tolist() == [2, 1, 1, 0]
    # the same with networks: one record per row and protocol
    nets = [cc._l4("n%d" % i, "10.%d.0.0/16" % i, "tcp", 0, 65535, dst="10.%d.0.0/%d" % (i % 7, 8 + i % 9))
            for i in range(12)]
    ref = td.diff_ref(nets, nets + allow, af)
    (ks, kd, kt, ku) = ref["dims"]
    assert (kt, ku) == (1, 1) and ref["n_rec"] >= ks * kd * 3
    _diff(eng, nets, nets + allow, af, want=ref, what="networks against allow-all behind them")


@pytest.mark.parametrize("af", _AFS)
def test_more_rules_than_the_folds_lds_bins(eng, af):
    """cover_fold counts in per-workgroup LDS bins up to 15,360 rules and in
    global memory above: 15,400 two-port TCP rules against the list with one
    rule deleted."""
    a = [cc._l4("p%d" % i, "", "tcp", 4 * i, 4 * i + 1) for i in range(15400)]
    b = a[:7000] + a[7001:]
    ref = td.diff_ref(a, b, af)
    assert len(b) + 2 > 15360 and ref["n_diff"] >= 1 and ref["cells_a"][7000] >= 1
    ta, tb = eng.put_table("big a", a), eng.put_table("big b", b)
    try:
        for tile in (2048, None):
            eng.set_option("cover_tile", tile)
            td.assert_equal(eng.table_diff(ta, tb, af=af), ref, "15400 rules, tile %s" % tile)
    finally:
        eng.set_option("cover_tile", None)
        eng.del_table(ta)
        eng.del_table(tb)
    # behind a rule for every TCP port, DENY in a and PERMIT in b: the TCP
    # columns are one run of 30,800 cells over eight chunks (the other record:
    # the protocols above 2, which the front rule takes as well)
    a2, b2 = [cc._l4("tcp", "", "tcp", 0, 65535, M.DENY)] + a, [cc._l4("tcp", "", "tcp", 0, 65535, M.PERMIT)] + b
    ref = td.diff_ref(a2, b2, af)
    assert ref["n_rec"] == 2 and ref["n_diff"] == ref["dims"][2] + 1 > 30000
    _diff(eng, a2, b2, af, want=ref, what="one run of every TCP column")


# ---- consistency with the shipped paths ---------------------------------------

@pytest.mark.parametrize("af", _AFS)
def test_consistent_with_classify(eng, af):
    a, b, _ = _parity_case(80, 0.0, af)
    conv = cc.mapped16 if af == 16 else (lambda x: np.ascontiguousarray(x, np.uint32))
    ta, tb = eng.put_table("cons a", a), eng.put_table("cons b", b)
    try:
        got = eng.table_diff(ta, tb, af=af)
        for wit, own in ((got["wit_a"], ta), (got["wit_b"], tb)):
            k = np.flatnonzero(wit["live"])
            assert len(k) >= 1
            pk = (conv(wit["src"][k]), conv(wit["dst"][k]), np.ascontiguousarray(wit["dport"][k]),
                  np.ascontiguousarray(wit["proto"][k]))
            (va, ha), (vb, hb) = eng.classify_rules(ta, *pk), eng.classify_rules(tb, *pk)
            assert np.array_equal(ha if own is ta else hb, k)          # every witness hits its own rule
            assert np.all(va != vb)                                    # ... and the two verdicts differ
        c = cc.cells(a + b)
        pk = (conv(c["src"]), conv(c["dst"]), c["dport"], c["proto"])
        va, vb = eng.classify(ta, *pk)[0], eng.classify(tb, *pk)[0]
        hist = np.bincount(4 * va.astype(np.int64) + vb, minlength=16).reshape(4, 4)
        assert np.array_equal(got["pairs"], hist.astype(np.uint64))
    finally:
        eng.del_table(ta)
        eng.del_table(tb)


# ---- device form ----------------------------------------------------------------

def test_device_form(eng):
    """torch outputs inside 64 padding elements on a side stream equal the
    host form and leave the padding alone; each misaligned pointer is refused."""
    import torch
    a, b, ref = _parity_case(80, 0.0, 4)
    ra, rb, cap = len(a) + 1, len(b) + 1, ref["n_rec"] + 5
    ta, tb = eng.put_table("dev a", a), eng.put_table("dev b", b)
    try:
        host = eng.table_diff(ta, tb)
        td.assert_equal(host, ref, "host form")
        pad = 64
        shapes = ((1,), (4, 4), (1, 4), (ra,), (ra, 4), (rb,), (rb, 4), (cap, 8), (1,))
        kinds = (torch.int64, torch.int64, torch.int32, torch.int64, torch.int32, torch.int64, torch.int32,
                 torch.int32, torch.int64)
        full = [torch.full((sh[0] + 2 * pad,) + sh[1:], -7, dtype=dt, device="cuda") for sh, dt in zip(shapes, kinds)]
        out = [t[pad:pad + sh[0]] for t, sh in zip(full, shapes)]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        for mode in ("auto", "linear"):
            got = eng.table_diff(ta, tb, mode=mode, rec_cap=cap, out=out, stream=side)
            assert got["n_cells"] == host["n_cells"] and got["dims"] == host["dims"]
            side.synchronize()
            h = [t.cpu().numpy() for t in out]
            assert int(h[0][0]) == host["n_diff"] and int(h[8][0]) == host["n_rec"]
            assert np.array_equal(h[1].view(np.uint64), host["pairs"])
            assert h[2].tobytes() == host["first"].tobytes()
            assert np.array_equal(h[3].view(np.uint64), host["cells_a"]) and h[4].tobytes() == host["wit_a"].tobytes()
            assert np.array_equal(h[5].view(np.uint64), host["cells_b"]) and h[6].tobytes() == host["wit_b"].tobytes()
            assert h[7][:host["n_rec"]].tobytes() == host["records"].tobytes()
            assert bool((out[7][host["n_rec"]:] == -7).all())          # beyond the records: untouched
            for t in full:
                assert bool((t[:pad] == -7).all()) and bool((t[-pad:] == -7).all())
        # misaligned device pointers: refused with nothing written
        L = _abi.lib()
        n_cells, dims = np.full(1, 77, np.uint64), np.full(4, 77, np.uint32)
        names = ("n_diff", "pairs_out", "first_out", "cells_a", "wit_a", "cells_b", "wit_b", "rec_out", "n_rec")
        ok = {k: t[pad:].data_ptr() for k, t in zip(names, full)}
        before = [t.clone() for t in full]
        for name, off in (("n_diff", 4), ("pairs_out", 4), ("first_out", 8), ("cells_a", 4), ("wit_a", 8),
                          ("wit_a", 4), ("cells_b", 4), ("wit_b", 8), ("rec_out", 8), ("rec_out", 4), ("n_rec", 4)):
            p = dict(ok, **{name: ok[name] + off})
            o = _abi.TDiffOut(*[p[k] for k in names[:8]], cap, p["n_rec"], n_cells.ctypes.data, dims.ctypes.data)
            assert L.cls_table_diff(eng.h, ta.id, tb.id, 4, C.byref(o), _abi.F_DEVICE, None) == _abi.E_INVAL, name
            torch.cuda.synchronize()
            assert n_cells[0] == 77 and np.all(dims == 77)
            assert all(bool((x == y).all()) for x, y in zip(before, full)), name
    finally:
        eng.del_table(ta)
        eng.del_table(tb)


# ---- refusals ------------------------------------------------------------------

def test_refusals_leave_the_outputs_alone(eng):
    from test_directed_traffic_cpu import refused_v16_table
    L = _abi.lib()
    a, b, ref = _parity_case(5, 0.0, 4)
    ta, tb = eng.put_table("ref a", a), eng.put_table("ref b", b)
    raw = _Raw(len(a) + 1, len(b) + 1, ref["n_rec"])
    none = {k: None for k in _Raw.ORDER[:8] + ("n_rec",)}
    cap = ref["n_rec"]
    try:
        o = raw.out(rec_cap=cap)
        for what, rc, args in (
                ("af 6", _abi.E_INVAL, (ta.id, tb.id, 6, C.byref(o), 0)),
                ("af 0", _abi.E_INVAL, (ta.id, tb.id, 0, C.byref(o), 0)),
                ("out NULL", _abi.E_INVAL, (ta.id, tb.id, 4, None, 0)),
                ("no output", _abi.E_INVAL, (ta.id, tb.id, 4, C.byref(raw.out(**none)), 0)),
                ("rec_out without n_rec", _abi.E_INVAL, (ta.id, tb.id, 4, C.byref(raw.out(rec_cap=cap, n_rec=None)), 0)),
                ("rec_cap without rec_out", _abi.E_INVAL, (ta.id, tb.id, 4, C.byref(raw.out(rec_cap=1, rec_out=None)), 0)),
                ("CLS_F_COUNT", _abi.E_INVAL, (ta.id, tb.id, 4, C.byref(o), _abi.F_COUNT)),
                ("CLS_F_NO_VERDICT", _abi.E_INVAL, (ta.id, tb.id, 4, C.byref(o), _abi.F_NO_VERDICT)),
                ("CLS_F_TIMING", _abi.E_INVAL, (ta.id, tb.id, 4, C.byref(o), _abi.F_TIMING)),
                ("CLS_F_CONN_CLS", _abi.E_INVAL, (ta.id, tb.id, 4, C.byref(o), _abi.F_CONN_CLS)),
                ("bit 31", _abi.E_INVAL, (ta.id, tb.id, 4, C.byref(o), 1 << 31)),
                ("unknown table a", _abi.E_NOTFOUND, (tb.id + 1000, tb.id, 4, C.byref(o), 0)),
                ("unknown table b", _abi.E_NOTFOUND, (ta.id, tb.id + 1000, 4, C.byref(o), 0))):
            assert L.cls_table_diff(eng.h, *args, None) == rc, what
            assert raw.untouched(), what
        # a V16 diff where either table has no 16-byte classifier; the message names the table
        t16 = eng.put_table("no16", refused_v16_table()[0])
        try:
            assert t16.info()["has_v16"] == 0
            for x, y in ((t16, tb), (ta, t16)):
                assert L.cls_table_diff(eng.h, x.id, y.id, 16, C.byref(o), 0, None) == _abi.E_INVAL
                msg = L.cls_last_error(eng.h).decode()
                assert "no 16-byte classifier" in msg and "(%d)" % t16.id in msg and raw.untouched(), msg
        finally:
            eng.del_table(t16)
        # the next valid call is unharmed
        td.assert_equal(eng.table_diff(ta, tb), ref, "after the refusals")
    finally:
        eng.del_table(ta)
        eng.del_table(tb)


def test_refusal_above_2_40_cells(eng):
    """cover's 4096-rule table (Ks = Kd = 8193, T = 16388: just above 2^40
    cells) against itself plus one rule.  The refusal precedes any device work,
    so nothing large runs."""
    L = _abi.lib()
    m = 4096
    ip = lambda x: "%d.%d.%d.%d/32" % (x >> 24, x >> 16 & 255, x >> 8 & 255, x & 255)
    rules = []
    for i in range(m):
        r = M.l4_rule(M.PERMIT, ip(0x0A000000 + 2 * i), ip(0x14000000 + 2 * i), "tcp", 0, 65535, 8 + 4 * i, 8 + 4 * i)
        r.matches.ip_rule.udp = M.Udp(destination_port_range=M.PortRange(9 + 4 * i, 9 + 4 * i),
                                      source_port_range=M.PortRange(0, 65535))
        rules.append(r)
    more = rules + [cc._l4("one more", ip(0x0A000000 + 2 * m), "tcp", 7, 7, dst=ip(0x14000000 + 2 * m))]
    ta, tb = eng.put_table("huge", rules), eng.put_table("huger", more)
    raw = _Raw(8, 8, 8)        # never written
    try:
        assert L.cls_table_diff(eng.h, ta.id, tb.id, 4, C.byref(raw.out(rec_cap=8)), 0, None) == _abi.E_INVAL
        msg = L.cls_last_error(eng.h).decode()
        assert "Ks 8195" in msg and "Kd 8195" in msg and "T 16389" in msg, msg
        assert raw.untouched()
    finally:
        eng.del_table(ta)
        eng.del_table(tb)


# ---- ACLEngine.acl_diff -----------------------------------------------------------

def test_acl_diff_on_a_rendered_scenario():
    """After every txn of one replayed renderer scenario: each installed ACL
    against its previous version (a rule list, put as a temporary table) and
    against itself, compared with the reference; no temporary table is left
    behind, also when the candidate list is refused."""
    from scenario_replay import load_scenarios, replay
    from vpp_amd._abi import ClsError
    from vpp_amd.engine import ACLEngine, Engine
    test = [t for t in load_scenarios() if t["name"] == "TestCombinedRules"][0]
    seen = {"acls": 0, "changed": 0}
    prev = {}

    def dotted(x):
        return "%d.%d.%d.%d" % (x >> 24, x >> 16 & 255, x >> 8 & 255, x & 255)

    def check(engine, calls):
        from test_directed_traffic_cpu import refused_v16_table
        e = engine.engine
        if not hasattr(e, "temp_tables"):                          # count the temporary tables put and deleted
            e.temp_tables = [0, 0]
            put, dele = e.put_table, e.del_table
            e.put_table = lambda *a: (e.temp_tables.__setitem__(0, e.temp_tables[0] + 1), put(*a))[1]
            e.del_table = lambda *a: (e.temp_tables.__setitem__(1, e.temp_tables[1] + 1), dele(*a))[1]
        for name, acl in engine.by_name.items():
            own = engine.acl_diff(name, name)
            assert own["equal"] and own["records"] == [] and own["rules_a"] == {} and own["rules_b"] == {}, name
            old = prev.get(name, [])
            ref = td.diff_ref(acl.rules, old)
            got = engine.acl_diff(name, old)
            assert got["equal"] == ref["equal"] and got["n_diff"] == ref["n_diff"], name
            assert got["n_cells"] == ref["n_cells"] and got["pairs"] == ref["pairs"].tolist(), name
            assert got["records"] == [
                ((dotted(int(r["src_lo"])), dotted(int(r["src_hi"])), dotted(int(r["dst_lo"])), dotted(int(r["dst_hi"]))),
                 int(r["proto"]), int(r["port_lo"]), int(r["port_hi"]), int(r["was"]), int(r["now"]),
                 int(r["rule_a"]), int(r["rule_b"])) for r in ref["records"]], name
            for side in "ab":
                w, c = ref["wit_" + side], ref["cells_" + side]
                assert got["rules_" + side] == {
                    k: (int(c[k]), (dotted(int(w[k]["src"])), dotted(int(w[k]["dst"])), int(w[k]["proto"]),
                                    int(w[k]["dport"]))) for k in range(len(w)) if w[k]["live"]}, (name, side)
            assert engine.acl_diff(name, old, af=16) == got, name
            seen["acls"] += 1
            seen["changed"] += not got["equal"]
        with pytest.raises(ClsError):
            engine.acl_diff("no such acl", [])
        if engine.by_name:
            name = next(iter(engine.by_name))
            with pytest.raises(ClsError):
                engine.acl_diff(name, "no such acl")
            before = e.temp_tables[0]
            with pytest.raises(ClsError):                              # a candidate refused after its put
                engine.acl_diff(name, refused_v16_table()[0], af=16)
            assert e.temp_tables[0] == before + 1
        assert e.temp_tables[0] == e.temp_tables[1] >= 1               # every temporary table is gone
        prev.clear()
        prev.update({name: list(acl.rules) for name, acl in engine.by_name.items()})
        return engine.connection_batch(calls)

    _, failures = replay(test, lambda contiv: ACLEngine(contiv, Engine()), check_conn=check)
    assert not failures, "\n".join(failures)
    assert seen["acls"] >= 2 and seen["changed"] >= 2


# ---- Go shims -------------------------------------------------------------------

@pytest.mark.parametrize("fam", [4, 16])
def test_go_shims_table_diff(fam, tmp_path, eng):
    """go/shimtest/tablediff (gcc): the diff through clsg_table_diff_v4 /
    clsg_table_diff_v16, as the Go binding's TableDiff calls them; its output
    files equal the reference."""
    from test_gpu_reach import _write_acls
    if not os.path.exists(TABLEDIFF):
        subprocess.run(["make", "-s", "-C", os.path.dirname(TABLEDIFF)], check=True)
    a, b, ref = _parity_case(80, 0.0, fam)
    _write_acls(tmp_path / "acls.txt", {"by_name": {"was": a, "now": b}, "ifs": ["if0"],
                                        "bind": {"if0": ("was", "now")}})
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(
        [os.path.join(ROOT, "vpp_amd")] + [x for x in [os.environ.get("LD_LIBRARY_PATH")] if x]))
    r = subprocess.run([TABLEDIFF, str(tmp_path), str(fam)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    u64 = lambda f: np.fromfile(tmp_path / f, "<u8")
    assert int(u64("out_tdiff_n.bin")[0]) == ref["n_diff"] and int(u64("out_tdiff_n.bin")[1]) == ref["n_rec"]
    assert int(u64("out_tdiff_n.bin")[2]) == ref["n_cells"]
    assert np.array_equal(u64("out_tdiff_pairs.bin").reshape(4, 4), ref["pairs"])
    assert (tmp_path / "out_tdiff_first.bin").read_bytes() == ref["first"].tobytes()
    assert np.array_equal(u64("out_tdiff_cells_a.bin"), ref["cells_a"])
    assert np.array_equal(u64("out_tdiff_cells_b.bin"), ref["cells_b"])
    assert (tmp_path / "out_tdiff_wit_a.bin").read_bytes() == ref["wit_a"].tobytes()
    assert (tmp_path / "out_tdiff_wit_b.bin").read_bytes() == ref["wit_b"].tobytes()
    assert (tmp_path / "out_tdiff_rec.bin").read_bytes() == ref["records"].tobytes()
    assert tuple(np.fromfile(tmp_path / "out_tdiff_dims.bin", "<u4")) == tuple(ref["dims"])
