"""The rule necessity sweep tests' shared helpers (tests/test_gpu_table_need.py,
tests/test_table_need_cpu.py), independent of the library's code: need_ref,
what cls_table_need reports, from the OpenMP oracle (oracle.classify_hits,
pinned to the literal evalACL by test_oracle_pin_cpu.py) over
cover_cases.cells(); need_literal, the definition taken literally on small
tables (the list without r against the list, over ALL cells); need_acl and
need_acl_fail, the constructed ACLs of named expectations; the large tables.
References are computed once per table and shared (ref)."""
import ctypes as C

import numpy as np

import cover_cases as cc
import oracle
from vpp_amd import _abi
from vpp_amd import model as M

SKIPPED, DEAD, REDUNDANT, NEEDED = 0, 1, 2, 3
MAX_CELLS = 1 << 16          # every table of these tests stays below this
FIELDS = ("src", "dst", "proto", "dport")


class _Sub:
    """The oracle's cls_rule array restricted to the rules ``idx`` (the
    strings stay the parent's): what the oracle compiles, as oracle.CRules."""

    def __init__(self, cr, idx):
        idx = np.asarray(idx, np.int64)
        self.n, self.parent = len(idx), cr
        self.arr = (oracle.ClsRule * max(1, self.n))()
        sz = C.sizeof(oracle.ClsRule)
        a = np.frombuffer(cr.arr, np.uint8).reshape(-1, sz)
        np.frombuffer(self.arr, np.uint8).reshape(-1, sz)[:self.n] = a[idx]

    def ptr(self):
        return C.cast(self.arr, C.POINTER(oracle.ClsRule))


def _classify(cr, idx, r, tr):
    """(ACLAction, terminating rule as an index into the full list of r rules;
    r: the default) of the packets tr under the rules ``idx`` of cr."""
    idx = np.asarray(idx, np.int64)
    v, h = oracle.classify_hits(_Sub(cr, idx), np.ascontiguousarray(tr["src"]), np.ascontiguousarray(tr["dst"]),
                                np.ascontiguousarray(tr["dport"]), np.ascontiguousarray(tr["proto"]))
    full = np.concatenate([idx, [r]]).astype(np.int64)
    return v, full[h.astype(np.int64)]


def need_ref(rules, skip=()):
    """What cls_table_need reports for ``rules`` with ``skip`` deleted: dict
    of need, free (uint8 [R]), first (uint64 [R+1]), changed (uint64 [R]),
    witness (_abi.NEED_WITNESS [R]), counts (uint32 [4]), n_cells, dims.
    first is the oracle over the cells; for each rule r that is first
    somewhere, the second match and the action after deletion come from the
    oracle over the list without r, restricted to r's cells."""
    r = len(rules)
    cr = oracle.rules_to_c(rules)
    c = cc.cells(rules)
    assert len(c["src"]) <= MAX_CELLS, len(c["src"])
    gone = set(int(k) for k in skip)
    kept = np.array([k for k in range(r) if k not in gone], np.int64)
    act, first = _classify(cr, kept, r, c)
    count = np.bincount(first, minlength=r + 1).astype(np.uint64)
    changed = np.zeros(r, np.uint64)
    second = np.full(len(first), r, np.int64)
    wit = np.zeros(r, _abi.NEED_WITNESS)
    need = np.zeros(r, np.uint8)
    for k in range(r):
        if k in gone:
            continue
        at = np.flatnonzero(first == k)
        if not len(at):
            need[k] = DEAD
            continue
        v2, h2 = _classify(cr, kept[kept != k], r, {f: c[f][at] for f in FIELDS})
        assert np.all(h2 > k)
        second[at] = h2
        diff = np.flatnonzero(v2 != act[at])
        changed[k] = len(diff)
        need[k] = NEEDED if len(diff) else REDUNDANT
        if len(diff):
            i = at[diff[0]]
            wit[k] = (c["src"][i], c["dst"][i], c["dport"][i], c["proto"][i], 0x80 | int(v2[diff[0]]), int(h2[diff[0]]))
    ok = np.concatenate([need == NEEDED, [True]])            # a second that stays: a needed rule, or the default
    chained = np.bincount(first[~ok[second]], minlength=r + 1)[:r]
    free = ((need == DEAD) | ((need == REDUNDANT) & (chained == 0))).astype(np.uint8)
    return dict(need=need, free=free, first=count, changed=changed, witness=wit,
                counts=np.bincount(need, minlength=4).astype(np.uint32), n_cells=len(first), dims=cc.dims(rules)[0])


def need_literal(rules):
    """The definition taken literally, for small lists: per rule r the list
    without r against the list over ALL cells of the list (a refinement of the
    shorter list's classes).  Returns (differing cells per rule, the least
    differing cell's packet and its action without r, or None)."""
    r = len(rules)
    assert r <= 40
    cr = oracle.rules_to_c(rules)
    c = cc.cells(rules)
    everything = np.arange(r)
    act, _ = _classify(cr, everything, r, c)
    out = []
    for k in range(r):
        v2, h2 = _classify(cr, everything[everything != k], r, c)
        diff = np.flatnonzero(v2 != act)
        least = None
        if len(diff):
            i = diff[0]
            least = (int(c["src"][i]), int(c["dst"][i]), int(c["dport"][i]), int(c["proto"][i]), 0x80 | int(v2[i]),
                     int(h2[i]))
        out.append((len(diff), least))
    return out


_REFS = {}


def ref(key, rules, skip=()):
    """need_ref, computed once per (key, skip) and shared; never modified."""
    k = (key, tuple(sorted(skip)))
    if k not in _REFS:
        _REFS[k] = need_ref(rules, skip)
    return _REFS[k]


def assert_equal(got, want, what=""):
    """Bit-exact equality of a host-form table_need result with need_ref's."""
    assert got["dims"] == tuple(want["dims"]) and got["n_cells"] == want["n_cells"], (what, got["dims"], want["dims"])
    for f in ("need", "free", "first", "changed", "counts"):
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero(got[f] != want[f])[:8], got[f][:12],
                                                 want[f][:12])
    bad = np.flatnonzero(got["witness"] != want["witness"])
    assert len(bad) == 0, (what, bad[:8], got["witness"][bad[:4]], want["witness"][bad[:4]])
    assert got["witness"].tobytes() == want["witness"].tobytes(), what
    assert int(got["first"].sum()) == got["n_cells"], what


def same_results(a, b, what=""):
    """Two host-form results are identical in every output."""
    assert a["dims"] == b["dims"] and a["n_cells"] == b["n_cells"], what
    for f in ("need", "free", "first", "changed", "counts"):
        assert np.array_equal(a[f], b[f]), (what, f)
    assert a["witness"].tobytes() == b["witness"].tobytes(), what


_l4 = cc._l4


def need_acl():
    """The constructed ACL of named expectations.  evalACL tests the networks
    first and, for protocols above 2, nothing else: a TCP rule also takes every
    such packet its networks contain.  Every group has a source /16 of its own."""
    return [
        # a /32 before its /24 on the same port: REDUNDANT, falls to the /24
        _l4("a32", "10.0.0.5/32", "tcp", 80, 80),
        _l4("a24", "10.0.0.0/24", "tcp", 80, 80),
        # the same pair with a DENY between them that overlaps the /32: NEEDED, witness the /32's low corner
        _l4("b32", "10.1.0.5/32", "tcp", 80, 80),
        _l4("bdeny", "10.1.0.0/28", "tcp", 80, 80, M.DENY),
        _l4("b24", "10.1.0.0/24", "tcp", 80, 80),
        # two /25 before their /24: the /24 is DEAD
        _l4("c25a", "10.2.0.0/25", "tcp", 0, 65535),
        _l4("c25b", "10.2.0.128/25", "tcp", 0, 65535),
        _l4("c24", "10.2.0.0/24", "tcp", 0, 65535, M.DENY),
        # PERMIT X twice: the first REDUNDANT but not free (it falls to a dead rule), the second DEAD and free
        _l4("d1", "10.3.0.0/16", "tcp", 443, 443),
        _l4("d2", "10.3.0.0/16", "tcp", 443, 443),
        # PERMIT before REFLECT on the same set: NEEDED, after REFLECT
        _l4("e1", "10.4.0.0/16", "tcp", 22, 22),
        _l4("e2", "10.4.0.0/16", "tcp", 22, 22, M.REFLECT),
        # a source-port FAILURE in front of a PERMIT: NEEDED
        _l4("f1", "10.5.0.0/16", "tcp", 0, 65535, sport=(0, 1000)),
        _l4("f2", "10.5.0.0/16", "tcp", 0, 65535),
        # live for protocols above 2 only: the witness has protocol 3
        _l4("g", "10.6.0.0/16", "tcp", 9, 8),
        # an IPv6 network: no IPv4 packet, DEAD in this sweep
        _l4("v6", "fd00:10::/64", "tcp", 80, 80),
        # the trailing deny-all, one rule per section: the last falls to the default alone and is free; the
        # one before it also falls to the last (protocols above 2) and is free only once that is gone
        _l4("deny_tcp", "", "tcp", 0, 65535, M.DENY),
        _l4("deny_udp", "", "udp", 0, 65535, M.DENY),
    ]


def need_acl_fail():
    """An unconditional FAILURE rule makes everything behind it DEAD; what is
    behind it still decides what takes over once it is deleted."""
    macip = M.Rule(actions=M.Actions(M.PERMIT), matches=M.Matches(macip_rule=M.MacIpRule()), rule_name="macip")
    return [_l4("x", "10.7.0.0/16", "tcp", 80, 80), macip, _l4("after_a", "", "tcp", 0, 65535),
            _l4("after_b", "10.8.0.0/16", "udp", 53, 53)]


def names(rules):
    return [r.rule_name for r in rules]


NETS = ["10.%d.0.0/16" % i for i in range(6)]
PORTS = [(80, 80), (443, 443), (1000, 1999), (5000, 5000)]


def strided_acl(n=4200):
    """n rules (W = 66 at 4,200: a lane of need_cells holds a second word) from
    six networks and four port ranges.  Placed: first and second in word 0
    (rules 0 and 1); first in word 0 and second in word 64, the same lane one
    stride on (rules 2 and 4100); first in word 63 and second in word 64
    (rules 4040 and 4110); a first match and no second (rule 3); cells with no
    match at all (every other network).  The rest repeat one (source,
    destination, port) triple: dead behind its first copy."""
    assert n >= 4200
    rules = [_l4("fill%d" % i, NETS[4], "tcp", *PORTS[0], dst=NETS[5]) for i in range(n)]
    rules[0] = _l4("w0a", NETS[0], "tcp", *PORTS[1])
    rules[1] = _l4("w0b", NETS[0], "tcp", *PORTS[1], M.DENY)
    rules[2] = _l4("w0_64a", NETS[1], "tcp", *PORTS[2])
    rules[4100] = _l4("w0_64b", NETS[1], "tcp", *PORTS[2], M.DENY)
    rules[4040] = _l4("w63_64a", NETS[2], "tcp", *PORTS[3])
    rules[4110] = _l4("w63_64b", NETS[2], "tcp", *PORTS[3])
    rules[3] = _l4("alone", NETS[3], "udp", *PORTS[0])
    return rules


def many_rules_acl(n=15400):
    """n rules over few classes (the sentinel fold's n_out = n + 2 above
    cover_fold's 15,360 LDS bins at 15,400): eight (network, port) triples in
    turn, so eight live rules in front and their copies dead behind them, then
    live rules of their own at the very end -- one needed, one redundant."""
    combos = [(NETS[i % 4], PORTS[i // 4 % 4]) for i in range(8)]
    rules = [_l4("r%d" % i, combos[i % 8][0], "tcp", *combos[i % 8][1]) for i in range(n)]
    rules[n - 3] = _l4("late_deny", NETS[4], "tcp", 80, 80, M.DENY)          # redundant: the default denies too
    rules[n - 2] = _l4("late_permit", NETS[5], "tcp", 80, 80)                # needed
    rules[n - 1] = _l4("late_shadow", NETS[5], "tcp", 80, 80, M.DENY)        # dead, and what late_permit falls to
    return rules
