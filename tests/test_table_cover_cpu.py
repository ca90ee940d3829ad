"""The rule coverage sweep without a GPU: cls_cover_classes against the
independent restatement (cover_cases.side_starts) on random rule lists with
malformed rules and on edge lists, and the soundness of the tests' own
reference (cover_cases.cover_ref) stated without any classes: whatever packet
the oracle sends to rule k, the reference calls k live and its witness is not
above that packet; every witness terminates at its own rule."""
import ctypes as C

import numpy as np
import pytest

import cover_cases as cc
from aclgen import random_acl, random_acl16, random_traffic
from reach_ext_cases import net_interval, rule_networks
from vpp_amd import _abi
from vpp_amd import model as M
from vpp_amd.engine import Engine


def _starts(rules, side):
    return Engine.cover_classes(rules, side).astype(np.int64)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("gen", [random_acl, random_acl16])
def test_cover_classes_random(gen, seed):
    rules, _ = gen(seed * 13 + 1, 120, 0.3)
    for side in (0, 1):
        got, want = _starts(rules, side), cc.side_starts(rules, side)
        assert np.array_equal(got, want), (side, got[:8], want[:8])
        assert got[0] == 0 and np.all(np.diff(got) > 0)
    # the two sides together are cls_addr_classes
    both = np.union1d(_starts(rules, 0), _starts(rules, 1))
    assert np.array_equal(both, Engine.addr_classes(rules).astype(np.int64))


def _rule(src, dst=""):
    return M.l4_rule(M.PERMIT, src, dst, "tcp", 0, 65535, 0, 65535)


@pytest.mark.parametrize("src,want", [
    ("0.0.0.0/0", [0]),
    ("0.0.0.0/32", [0, 1]),
    ("255.255.255.255/32", [0, 0xFFFFFFFF]),                     # no start at 2^32
    ("::ffff:10.0.0.0/104", [0, 10 << 24, 11 << 24]),            # IPv4-mapped: family 4
    ("fd00:10::/64", [0]), ("::/0", [0]), ("2001:db8::1/128", [0]),   # family 16: nothing
    ("garbage", [0]), ("10.0.0.0/33", [0]), ("", [0]),
    ("10.1.2.3/24", [0, 0x0A010200, 0x0A010300]),                # host bits masked
])
def test_cover_classes_edges(src, want):
    rules = [_rule(src, "192.168.0.0/16")]
    assert _starts(rules, 0).tolist() == want
    assert cc.side_starts(rules, 0).tolist() == want
    # the other side sees only its own network
    assert _starts(rules, 1).tolist() == [0, 0xC0A80000, 0xC0A90000]
    assert _starts([_rule("192.168.0.0/16", src)], 1).tolist() == want


def test_cover_classes_cap_and_refusals():
    rules, _ = random_acl(5, 60, 0.3)
    cr = _abi.CRules(rules)
    L = _abi.lib()
    want = cc.side_starts(rules, 0)
    n = C.c_uint32(0)
    lo = np.full(len(want), 0xA5A5A5A5, np.uint32)
    assert L.cls_cover_classes(cr.ptr(), cr.n, 0, lo.ctypes.data, len(want) - 1, C.byref(n)) == 0
    assert n.value == len(want) and np.all(lo == 0xA5A5A5A5)     # cap < K sets only *n
    assert L.cls_cover_classes(cr.ptr(), cr.n, 0, lo.ctypes.data, len(want), C.byref(n)) == 0
    assert np.array_equal(lo.astype(np.int64), want)
    assert L.cls_cover_classes(cr.ptr(), cr.n, 2, lo.ctypes.data, len(want), C.byref(n)) == _abi.E_INVAL
    assert L.cls_cover_classes(cr.ptr(), cr.n, 0, None, 0, None) == _abi.E_INVAL
    assert L.cls_cover_classes(None, 0, 1, None, 0, C.byref(n)) == 0 and n.value == 1


def _corners(rules, pool, seed):
    """Every network's lo - 1, lo, hi, hi + 1 (a sample of 64 per side)
    crossed with the rules' port ends (a sample of 32) and five protocols."""
    rng = np.random.default_rng(seed)
    a = {0, 0xFFFFFFFF}
    for s in rule_networks(rules):
        iv = net_interval(s)
        if iv is not None:
            a.update(x & 0xFFFFFFFF for x in (iv[0] - 1, iv[0], iv[1], iv[1] + 1))
    ports = {0, 65535}
    for r in rules:
        ipr = r.matches.ip_rule if r.matches is not None else None
        for l4 in ((ipr.tcp, ipr.udp) if ipr is not None else ()):
            rg = l4.destination_port_range if l4 is not None else None
            if rg is not None:
                for x in (rg.lower_port - 1, rg.lower_port, rg.upper_port, rg.upper_port + 1):
                    ports.add(x & 0xFFFF)
    a, ports = np.array(sorted(a), np.uint32), np.array(sorted(ports), np.uint16)
    sa = rng.choice(a, min(64, len(a)), replace=False)
    da = rng.choice(a, min(64, len(a)), replace=False)
    pt = rng.choice(ports, min(32, len(ports)), replace=False)
    pr = np.array([0, 1, 2, 3, 17], np.uint8)
    g = np.meshgrid(sa, da, pr, pt, indexing="ij")
    return dict(src=g[0].ravel(), dst=g[1].ravel(), proto=g[2].ravel(), dport=g[3].ravel())


@pytest.mark.parametrize("af", [4, 16])
@pytest.mark.parametrize("seed,weird", [(1, 0.0), (2, 0.3), (3, 0.3)])
def test_cover_ref_is_sound_without_classes(seed, weird, af):
    rules, pool = random_acl(seed * 7 + 2, 80, weird)
    rules = cc.shadowed_tail(rules, seed)
    ref = cc.cover_ref(rules, af)
    w = ref["witness"]
    assert ref["n_dead"] >= 1 and int(ref["live"].sum()) >= 2
    assert int(ref["cells"].sum()) == ref["n_cells"] == cc.dims(rules)[1]
    tr = random_traffic(seed + 90, 200000, pool)
    co = _corners(rules, pool, seed)
    tr = {k: np.concatenate([tr[k], co[k]]) for k in ("src", "dst", "proto", "dport")}
    hit = cc.oracle_rules(rules, tr, af)
    assert np.all(ref["live"][hit] == 1)
    ws, wd, wp, wq = (w[f][hit].astype(np.int64) for f in ("src", "dst", "proto", "dport"))
    s, d, q = (tr[f].astype(np.int64) for f in ("src", "dst", "dport"))
    p = np.minimum(tr["proto"].astype(np.int64), 3)
    le = (ws < s) | ((ws == s) & ((wd < d) | ((wd == d) & ((wp < p) | ((wp == p) & (wq <= q))))))
    assert np.all(le), np.flatnonzero(~le)[:8]
    # every witness terminates at its own rule; dead rules have all-zero records
    k = np.flatnonzero(ref["live"])
    own = cc.oracle_rules(rules, {f: np.ascontiguousarray(w[f][k]) for f in ("src", "dst", "proto", "dport")}, af)
    assert np.array_equal(own, k)
    dead = w[ref["live"] == 0]
    assert dead.tobytes() == bytes(16 * len(dead))


def test_shadow_acl_reference():
    """The constructed shadows on the oracle alone: the dead set by name."""
    rules, dead = cc.shadow_acl()
    ref = cc.cover_ref(rules)
    names = [r.rule_name for r in rules]
    assert [names[k] for k in np.flatnonzero(ref["live"][:-1] == 0)] == dead
    assert ref["live"][-1] == 0                                  # behind macip nothing reaches the default
    w = ref["witness"]
    at = names.index
    assert tuple(w[at("tcp_other_only")])[:5] == (10 << 24 | 2 << 16, 0, 0, 3, 1)
    assert tuple(w[at("sport_fail")])[:5] == (10 << 24 | 3 << 16, 0, 0, 0, 1)
    assert tuple(w[at("bad_dst")])[:5] == (10 << 24 | 4 << 16, 0, 0, 0, 1)
    assert tuple(w[at("icmp")])[:5] == (0, 0, 0, 2, 1)
    assert tuple(w[at("macip")])[:5] == (0, 0, 0, 0, 1)
