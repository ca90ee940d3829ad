"""The table diff tests' shared helpers (tests/test_gpu_table_diff.py,
tests/test_table_diff_cpu.py), all independent of the library's code: diff_ref,
the OpenMP oracle (oracle.classify_hits) under both rule lists over
cover_cases.cells of the two lists concatenated, reduced with numpy to what
cls_table_diff reports (records from run boundaries); assert_equal, bit-exact;
edit, a second list that differs (edits of live rules, chosen from cover_ref);
equivalent, rewrites without a semantic change."""
import copy

import numpy as np

import cover_cases as cc
import oracle
from vpp_amd import _abi
from vpp_amd import model as M

FIELDS = ("src", "dst", "proto", "dport")


def verdicts(rules, tr, af=4):
    """(ACLAction uint8, terminating rule int64) of each packet of tr under rules."""
    src, dst = (cc.mapped16(tr["src"]), cc.mapped16(tr["dst"])) if af == 16 else (tr["src"], tr["dst"])
    v, h = oracle.classify_hits(oracle.rules_to_c(rules), np.ascontiguousarray(src), np.ascontiguousarray(dst),
                                tr["dport"], tr["proto"], af=af)
    return v, h.astype(np.int64)


def _witness(c, at):
    w = np.zeros(len(at), _abi.COVER_WITNESS)
    for f in FIELDS:
        w[f] = c[f][at]
    w["live"] = 1
    return w


def _side(hit, diff, r, c):
    """Per rule of one table: the differing cells terminating there and the least one's packet."""
    at = np.flatnonzero(diff)
    count = np.bincount(hit[at], minlength=r + 1).astype(np.uint64)
    assert len(count) == r + 1
    wit = np.zeros(r + 1, _abi.COVER_WITNESS)
    k, first = np.unique(hit[at], return_index=True)
    wit[k] = _witness(c, at[first])
    return count, wit


def diff_ref(a, b, af=4):
    """What cls_table_diff reports for rule lists a and b, from the oracle over
    the cells of a + b: dict of equal, n_diff, pairs, first, cells_a, wit_a,
    cells_b, wit_b, records (_abi.TDIFF_REC, all of them), n_rec, n_cells,
    dims; and mask, whether each cell differs (for the tests' own shapes)."""
    both = list(a) + list(b)
    c = cc.cells(both)
    (ks, kd, kt, ku), n = cc.dims(both)
    t = kt + ku + 2
    va, ha = verdicts(a, c, af)
    vb, hb = verdicts(b, c, af)
    diff = va != vb
    pairs = np.bincount(4 * va.astype(np.int64) + vb, minlength=16).astype(np.uint64).reshape(4, 4)
    first = np.zeros(1, _abi.COVER_WITNESS)
    if diff.any():
        first = _witness(c, np.flatnonzero(diff)[:1])
    cells_a, wit_a = _side(ha, diff, len(a), c)
    cells_b, wit_b = _side(hb, diff, len(b), c)
    # runs: consecutive differing cells of one row and one protocol with equal (was, now, rule_a, rule_b)
    idx = np.arange(n, dtype=np.int64)
    j = idx % t
    seg = (idx // t) * 4 + (j >= kt).astype(np.int64) + (j >= kt + ku) + (j >= kt + ku + 1)
    same = np.zeros(n, bool)          # cell i continues the run of cell i - 1
    same[1:] = (diff[1:] & diff[:-1] & (seg[1:] == seg[:-1]) & (va[1:] == va[:-1]) & (vb[1:] == vb[:-1]) &
                (ha[1:] == ha[:-1]) & (hb[1:] == hb[:-1]))
    head = np.flatnonzero(diff & ~same)
    tail = np.flatnonzero(diff & ~np.append(same[1:], False))
    assert len(head) == len(tail) and np.all(head <= tail) and np.all(seg[head] == seg[tail])
    slo, dlo = cc.side_starts(both, 0), cc.side_starts(both, 1)
    _, dport, _, _ = cc.columns(both)
    s, d, jt = head // (kd * t), head // t % kd, j[tail]
    rec = np.zeros(len(head), _abi.TDIFF_REC)
    rec["src_lo"], rec["dst_lo"] = slo[s], dlo[d]
    rec["src_hi"] = np.append(slo[1:] - 1, 0xFFFFFFFF)[s]
    rec["dst_hi"] = np.append(dlo[1:] - 1, 0xFFFFFFFF)[d]
    rec["port_lo"] = c["dport"][head]
    seg_last = (jt == kt - 1) | (jt >= kt + ku - 1)             # the tail is its protocol's last column
    rec["port_hi"] = np.where(seg_last, 65535, np.append(dport[1:].astype(np.int64) - 1, 65535)[jt])
    rec["proto"] = c["proto"][head]
    rec["was"], rec["now"], rec["rule_a"], rec["rule_b"] = va[head], vb[head], ha[head], hb[head]
    return dict(equal=not diff.any(), n_diff=int(diff.sum()), pairs=pairs, first=first[0], cells_a=cells_a,
                wit_a=wit_a, cells_b=cells_b, wit_b=wit_b, records=rec, n_rec=len(rec), n_cells=n,
                dims=(ks, kd, kt, ku), mask=diff)


def assert_equal(got, want, what="", rec_cap=None):
    """Bit-exact equality of a host-form Engine.table_diff result with diff_ref's
    (rec_cap: the records are the first min(rec_cap, n_rec))."""
    assert got["dims"] == tuple(want["dims"]) and got["n_cells"] == want["n_cells"], (what, got["dims"], want["dims"])
    assert got["n_diff"] == want["n_diff"] and got["equal"] == want["equal"], (what, got["n_diff"], want["n_diff"])
    assert np.array_equal(got["pairs"], want["pairs"]), (what, got["pairs"], want["pairs"])
    assert int(got["pairs"].sum()) == got["n_cells"], what
    assert got["first"].tobytes() == want["first"].tobytes(), (what, got["first"], want["first"])
    for side in "ab":
        g, w = got["cells_" + side], want["cells_" + side]
        assert np.array_equal(g, w), (what, side, np.flatnonzero(g != w)[:8])
        assert int(g.sum()) == got["n_diff"], (what, side)
        g, w = got["wit_" + side], want["wit_" + side]
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, side, bad[:8], g[bad[:4]], w[bad[:4]])
        assert g.tobytes() == w.tobytes(), (what, side)
    assert got["n_rec"] == want["n_rec"], (what, got["n_rec"], want["n_rec"])
    keep = want["n_rec"] if rec_cap is None else min(rec_cap, want["n_rec"])
    g, w = got["records"], want["records"][:keep]
    assert len(g) == len(w), (what, len(g), len(w))
    bad = np.flatnonzero(g != w)
    assert len(bad) == 0, (what, bad[:8], g[bad[:3]], w[bad[:3]])
    assert g.tobytes() == w.tobytes(), what


# ---- second lists ---------------------------------------------------------------

def live_rules(rules, af=4):
    """The rules with action PERMIT or DENY that some packet terminates at
    with that action, by cells descending (cover_ref and the oracle's verdict
    of each one's witness)."""
    ref = cc.cover_ref(rules, af)
    w = ref["witness"]
    v, h = verdicts(rules, {f: np.ascontiguousarray(w[f]) for f in FIELDS}, af)
    ks = [k for k in range(len(rules)) if ref["live"][k] and h[k] == k and rules[k].actions is not None and
          rules[k].actions.acl_action in (M.PERMIT, M.DENY) and v[k] == rules[k].actions.acl_action]
    return sorted(ks, key=lambda k: (-int(ref["cells"][k]), k))


def edit(rules, af=4):
    """A list that differs from rules: PERMIT <-> DENY on the live PERMIT /
    DENY rule with the most cells, the next such rule deleted, and a new DENY
    rule with networks and ports of its own in front.  (Edits of random rules
    hit dead ones and change nothing.)"""
    ks = live_rules(rules, af)
    assert ks, "no live PERMIT / DENY rule"
    out = [copy.deepcopy(r) for r in rules]
    act = out[ks[0]].actions
    act.acl_action = M.DENY if act.acl_action == M.PERMIT else M.PERMIT
    if len(ks) > 1:
        del out[ks[1]]
    return [cc._l4("front", "198.51.100.0/24", "tcp", 1000, 2000, M.DENY, dst="203.0.113.0/25")] + out


def _net24(s):
    iv = cc.net_interval(s)
    return iv is not None and "." in s and s.endswith("/24") and iv[1] - iv[0] == 255


def equivalent(rules):
    """rules rewritten with no semantic change: the first rule with a /24
    source replaced by its two /25 halves, the first two neighbours with
    disjoint source networks swapped, and a dead duplicate of the first rule
    appended."""
    out = [copy.deepcopy(r) for r in rules]
    srcs = [r.matches.ip_rule.ip.source_network if r.matches is not None and r.matches.ip_rule is not None and
            r.matches.ip_rule.ip is not None else None for r in out]
    done = {"split": False, "swap": False}
    for k in range(len(out) - 1):
        a, b = (cc.net_interval(s) if s else None for s in srcs[k:k + 2])
        if a is not None and b is not None and (a[1] < b[0] or b[1] < a[0]):
            out[k], out[k + 1] = out[k + 1], out[k]
            srcs[k], srcs[k + 1] = srcs[k + 1], srcs[k]
            done["swap"] = True
            break
    starts = set(cc.side_starts(rules, 0).tolist())
    for k, s in enumerate(srcs):
        if s and _net24(s) and cc.net_interval(s)[0] + 128 not in starts:      # the halves add a class
            lo = cc.net_interval(s)[0]
            ip = lambda x: "%d.%d.%d.%d/25" % (x >> 24, x >> 16 & 255, x >> 8 & 255, x & 255)
            halves = [copy.deepcopy(out[k]), copy.deepcopy(out[k])]
            halves[0].matches.ip_rule.ip.source_network = ip(lo)
            halves[1].matches.ip_rule.ip.source_network = ip(lo + 128)
            out[k:k + 1] = halves
            done["split"] = True
            break
    if out:
        out.append(copy.deepcopy(out[0]))
    return out, done
