"""The table diff without a GPU: the ABI's structs and symbol, and the
soundness of the tests' own reference (table_diff_cases.diff_ref) stated
without any classes: whatever packet the oracle gives two different verdicts
under the two lists lies in exactly one record, which carries the packet's
verdicts and terminating rules, and `first` is not above it; rewrites without a
semantic change give no difference although the classes change; a dead rule
with new networks changes the records but not the canonical outputs."""
import copy
import ctypes as C

import numpy as np
import pytest

import cover_cases as cc
import table_diff_cases as td
from aclgen import random_acl, random_acl16
from vpp_amd import _abi


def test_abi_structs_and_symbol():
    assert _abi.TDIFF_REC.itemsize == 32 and _abi.COVER_WITNESS.itemsize == 16
    assert C.sizeof(_abi.TDiffOut) == 12 * 8
    assert "cls_table_diff" in _abi.SYMBOLS
    assert _abi.lib().cls_table_diff.argtypes[4] == C.POINTER(_abi.TDiffOut)


def _sample(both, n, seed):
    """n packets biased to the class edges of `both` and the values next to them."""
    rng = np.random.default_rng(seed)

    def draw(edges, top, dtype):
        e = np.asarray(edges, np.int64)
        near = (rng.choice(e, n) + rng.integers(-1, 2, n)) % (top + 1)
        return np.where(rng.random(n) < 0.8, near, rng.integers(0, top + 1, n)).astype(dtype)
    _, _, kt, ku = cc.columns(both)
    ports = cc.columns(both)[1][:kt + ku]
    return dict(src=draw(cc.side_starts(both, 0), 0xFFFFFFFF, np.uint32),
                dst=draw(cc.side_starts(both, 1), 0xFFFFFFFF, np.uint32), dport=draw(ports, 65535, np.uint16),
                proto=rng.choice(np.array([0, 1, 2, 3, 17, 255], np.uint8), n, p=[.35, .35, .1, .1, .05, .05]))


def _differing(a, b, tr, af):
    (va, ha), (vb, hb) = td.verdicts(a, tr, af), td.verdicts(b, tr, af)
    return va != vb, va, vb, ha, hb


def _containing(rec, tr):
    """(records containing each packet, the index of one of them)."""
    s, d, q = (tr[f].astype(np.int64)[:, None] for f in ("src", "dst", "dport"))
    p = np.minimum(tr["proto"].astype(np.int64), 3)[:, None]
    count, which = np.zeros(len(s), np.int64), np.full(len(s), -1, np.int64)
    for i in range(0, len(rec), 64):
        r = {f: rec[f][i:i + 64].astype(np.int64)[None, :] for f in rec.dtype.names}
        m = ((s >= r["src_lo"]) & (s <= r["src_hi"]) & (d >= r["dst_lo"]) & (d <= r["dst_hi"]) & (p == r["proto"]) &
             (q >= r["port_lo"]) & (q <= r["port_hi"]))
        count += m.sum(1)
        which = np.where(m.any(1), i + m.argmax(1), which)
    return count, which


def _le(w, tr):
    """Witness w <= each packet of tr in (src, dst, proto, dport) order, protocol 3 for every value above 2."""
    ws, wd, wp, wq = (int(w[f]) for f in ("src", "dst", "proto", "dport"))
    s, d, q = (tr[f].astype(np.int64) for f in ("src", "dst", "dport"))
    p = np.minimum(tr["proto"].astype(np.int64), 3)
    return (ws < s) | ((ws == s) & ((wd < d) | ((wd == d) & ((wp < p) | ((wp == p) & (wq <= q))))))


@pytest.mark.parametrize("af,seed,n,weird", [(4, 241, 80, 0.0), (4, 244, 80, 0.3), (16, 241, 80, 0.0)])
def test_diff_ref_is_sound_without_classes(af, seed, n, weird):
    a = cc.shadowed_tail((random_acl16 if af == 16 else random_acl)(seed, n, weird)[0], n)
    b = td.edit(a, af)
    ref = td.diff_ref(a, b, af)
    assert 1 <= ref["n_diff"] < ref["n_cells"] and ref["n_rec"] >= 2
    assert int(ref["pairs"].sum()) == ref["n_cells"] and ref["first"]["live"] == 1
    tr = _sample(a + b, 200000, seed)
    diff, va, vb, ha, hb = _differing(a, b, tr, af)
    assert diff.any() and not diff.all()
    count, which = _containing(ref["records"], tr)
    assert np.array_equal(count, diff.astype(np.int64)), np.flatnonzero(count != diff)[:8]
    r = ref["records"][which[diff]]
    for f, v in (("was", va), ("now", vb), ("rule_a", ha), ("rule_b", hb)):
        assert np.array_equal(r[f].astype(np.int64), v[diff].astype(np.int64)), f
    assert np.all(r["was"] != r["now"])
    hit = {f: tr[f][diff] for f in td.FIELDS}
    assert np.all(_le(ref["first"], hit))
    # per side: the rule's witness is not above any differing packet terminating there
    for wit, h in ((ref["wit_a"], ha[diff]), (ref["wit_b"], hb[diff])):
        for k in np.unique(h):
            assert wit[k]["live"] == 1 and np.all(_le(wit[k], {f: hit[f][h == k] for f in td.FIELDS})), k


@pytest.mark.parametrize("seed", [16, 77])
def test_equivalent_rewrites_change_the_classes_only(seed):
    a = cc.shadowed_tail(random_acl(seed, 60, 0.0)[0], 5)
    e, done = td.equivalent(a)
    assert done == {"split": True, "swap": True} and len(e) == len(a) + 2
    ref = td.diff_ref(a, e)
    assert ref["equal"] and ref["n_diff"] == 0 and ref["n_rec"] == 0 and ref["first"]["live"] == 0
    assert tuple(ref["dims"]) != tuple(cc.dims(a)[0])
    assert np.array_equal(ref["pairs"], np.diag(np.diag(ref["pairs"])))


def test_a_dead_rule_with_new_networks_moves_only_the_records():
    a = cc.shadowed_tail(random_acl(241, 80, 0.0)[0], 80)
    b = td.edit(a)
    ref = td.diff_ref(a, b)
    # a copy of the rule a record terminates at in b, narrowed to one source
    # address inside the record: dead behind the original, and its /32 cuts the
    # record's source class in three
    r0 = [r for r in ref["records"] if r["rule_b"] < len(b) and int(r["src_hi"]) - int(r["src_lo"]) >= 2][0]
    dead = copy.deepcopy(b[int(r0["rule_b"])])
    x = int(r0["src_lo"]) + 1
    dead.matches.ip_rule.ip.source_network = "%d.%d.%d.%d/32" % (x >> 24, x >> 16 & 255, x >> 8 & 255, x & 255)
    b2 = b + [dead]
    ref2 = td.diff_ref(a, b2)
    assert ref2["dims"] != ref["dims"] and ref2["n_rec"] != ref["n_rec"]
    assert ref2["first"].tobytes() == ref["first"].tobytes()
    assert ref2["wit_a"].tobytes() == ref["wit_a"].tobytes()
    assert ref2["wit_b"][:len(b)].tobytes() == ref["wit_b"][:len(b)].tobytes()
    assert ref2["wit_b"][len(b)]["live"] == 0 and ref2["cells_b"][len(b)] == 0          # dead: no differing cell
    assert ref2["wit_b"][len(b) + 1].tobytes() == ref["wit_b"][len(b)].tobytes()         # the default
    tr = _sample(a + b2, 200000, 5)
    d1, d2 = _differing(a, b, tr, 4)[0], _differing(a, b2, tr, 4)[0]
    assert np.array_equal(d1, d2) and d1.any()
