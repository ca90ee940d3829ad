"""The rule coverage sweep tests' shared helpers (tests/test_gpu_table_cover.py,
tests/test_table_cover_cpu.py), all independent of the library's code:
side_starts, the IPv4 address class starts of one side of a rule list from
model.Rule objects (vpp_amd.gonet's ParseCIDR and networkNumberAndMask, as
reach_ext_cases.net_interval); columns, the (protocol, port) columns; cells,
the representative packets in cell order; cover_ref, the OpenMP oracle
(oracle.classify_hits, pinned to the literal evalACL by
test_oracle_pin_cpu.py) over those cells reduced with numpy to what
cls_table_cover reports; shadow_acl, the constructed ACL of named shadows."""
import numpy as np

import oracle
from reach_ext_cases import net_interval
from reach_ports_cases import class_starts as port_starts
from vpp_amd import _abi
from vpp_amd import model as M

MAX_CELLS = 1 << 22          # the tests keep every table at or below this


def side_starts(rules, side):
    """The class starts of the source (side 0) or destination (side 1)
    networks: 0, and lo and hi + 1 <= 2^32 - 1 of every network of that side
    that holds IPv4 addresses; ascending int64."""
    s = {0}
    for r in rules:
        ipr = r.matches.ip_rule if r.matches is not None else None
        ip = ipr.ip if ipr is not None else None
        if ip is None:
            continue
        iv = net_interval(ip.destination_network if side else ip.source_network)
        if iv is not None:
            s.add(iv[0])
            if iv[1] < 0xFFFFFFFF:
                s.add(iv[1] + 1)
    return np.array(sorted(s), np.int64)


def columns(rules):
    """(proto uint8 [T], dport uint16 [T], Kt, Ku): the TCP port classes
    ascending, the UDP port classes, one ICMP column (port 0), one column for
    every other protocol (protocol 3, port 0)."""
    t, u = port_starts([rules], 0), port_starts([rules], 1)
    proto = np.concatenate([np.zeros(len(t)), np.ones(len(u)), [2, 3]]).astype(np.uint8)
    dport = np.concatenate([t, u, [0, 0]]).astype(np.uint16)
    return proto, dport, len(t), len(u)


def dims(rules):
    """(Ks, Kd, Kt, Ku) and the cell count Ks Kd T."""
    ks, kd = len(side_starts(rules, 0)), len(side_starts(rules, 1))
    _, _, kt, ku = columns(rules)
    return (ks, kd, kt, ku), ks * kd * (kt + ku + 2)


def cells(rules):
    """The representative packets in cell order, cell = (s Kd + d) T + j:
    dict of src, dst (uint32), proto (uint8), dport (uint16)."""
    slo, dlo = side_starts(rules, 0), side_starts(rules, 1)
    proto, dport, _, _ = columns(rules)
    ks, kd, t = len(slo), len(dlo), len(proto)
    assert ks * kd * t <= MAX_CELLS, (ks, kd, t)
    return dict(src=np.repeat(slo, kd * t).astype(np.uint32), dst=np.tile(np.repeat(dlo, t), ks).astype(np.uint32),
                proto=np.tile(proto, ks * kd), dport=np.tile(dport, ks * kd))


def mapped16(a):
    """IPv4 addresses (host-order uint32) as the 16 network-order bytes of ::ffff:a."""
    a = np.ascontiguousarray(a, np.uint32)
    out = np.zeros((len(a), 16), np.uint8)
    out[:, 10:12] = 0xFF
    out[:, 12:] = a.astype(">u4").view(np.uint8).reshape(-1, 4)
    return out


def oracle_rules(rules, tr, af=4):
    """The oracle's terminating rule of each packet of tr (R: the default)."""
    src, dst = (mapped16(tr["src"]), mapped16(tr["dst"])) if af == 16 else (tr["src"], tr["dst"])
    return oracle.classify_hits(oracle.rules_to_c(rules), np.ascontiguousarray(src), np.ascontiguousarray(dst),
                                tr["dport"], tr["proto"], af=af)[1]


def cover_ref(rules, af=4):
    """What cls_table_cover reports, from the oracle over cells(rules): dict
    of live uint8 [R+1], witness (_abi.COVER_WITNESS [R+1]), cells uint64
    [R+1], n_dead, n_cells, dims."""
    c = cells(rules)
    hit = oracle_rules(rules, c, af).astype(np.int64)
    r = len(rules)
    count = np.bincount(hit, minlength=r + 1).astype(np.uint64)
    assert len(count) == r + 1
    live = (count > 0).astype(np.uint8)
    wit = np.zeros(r + 1, _abi.COVER_WITNESS)
    k, first = np.unique(hit, return_index=True)          # the first (lowest) cell of each rule hit
    for f in ("src", "dst", "dport", "proto"):
        wit[f][k] = c[f][first]
    wit["live"][k] = 1
    return dict(live=live, witness=wit, cells=count, n_dead=int((live[:r] == 0).sum()), n_cells=len(hit),
                dims=dims(rules)[0])


def assert_equal(got, want, what=""):
    """Bit-exact equality of a host-form Engine.table_cover result with cover_ref's."""
    assert got["dims"] == tuple(want["dims"]) and got["n_cells"] == want["n_cells"], (what, got["dims"], want["dims"])
    assert np.array_equal(got["live"], want["live"]), (what, np.flatnonzero(got["live"] != want["live"])[:8])
    bad = np.flatnonzero(got["witness"] != want["witness"])
    assert len(bad) == 0, (what, bad[:8], got["witness"][bad[:4]], want["witness"][bad[:4]])
    assert got["witness"].tobytes() == want["witness"].tobytes(), what
    assert np.array_equal(got["cells"], want["cells"]), (what, np.flatnonzero(got["cells"] != want["cells"])[:8])
    assert int(got["cells"].sum()) == got["n_cells"], what
    assert got["n_dead"] == want["n_dead"], (what, got["n_dead"], want["n_dead"])


def _l4(name, src, proto, lo, hi, action=M.PERMIT, dst="", sport=(0, 65535)):
    r = M.l4_rule(action, src, dst, proto, sport[0], sport[1], lo, hi)
    r.rule_name = name
    return r


def shadow_acl():
    """(rules, the names of the dead rules).  evalACL tests the networks
    first and, for protocols above 2, nothing else: a rule takes every such
    packet its networks contain, whatever its sections say.  So a range with
    lo > hi is dead only where earlier rules contain its networks (`empty`);
    on networks of its own it is live for protocols above 2 alone
    (`tcp_other_only`: witness protocol 3)."""
    rules = [
        _l4("half_lo", "10.0.0.0/25", "tcp", 0, 65535),
        _l4("half_hi", "10.0.0.128/25", "tcp", 0, 65535),
        _l4("whole24", "10.0.0.0/24", "tcp", 0, 65535, M.DENY),          # dead: the union of the two halves
        _l4("ports_a", "10.1.0.0/16", "udp", 100, 200),
        _l4("ports_b", "10.1.0.0/16", "udp", 201, 300),
        _l4("ports_in_union", "10.1.0.0/16", "udp", 150, 250, M.DENY),   # dead: inside 100 .. 300
        _l4("dup", "10.1.0.0/16", "udp", 100, 200),                      # dead: ports_a again
        _l4("empty", "10.1.0.0/16", "udp", 500, 400),                    # dead: no port, and ports_a takes protocols > 2
        _l4("tcp_other_only", "10.2.0.0/16", "tcp", 9, 8),               # live for protocols > 2 only
        _l4("sport_fail", "10.3.0.0/16", "tcp", 0, 65535, sport=(0, 1000)),   # live: FAILURE at the rule
        _l4("bad_dst", "10.4.0.0/16", "tcp", 80, 80, dst="garbage"),     # live: FAILURE at the rule
    ]
    icmp = M.icmp_rule(M.PERMIT)
    icmp.rule_name = "icmp"
    macip = M.Rule(actions=M.Actions(M.PERMIT), matches=M.Matches(macip_rule=M.MacIpRule()), rule_name="macip")
    rules += [icmp, macip, _l4("after_fail", "", "tcp", 0, 65535)]       # dead: behind the unconditional FAILURE
    return rules, ["whole24", "ports_in_union", "dup", "empty", "after_fail"]


def shadowed_tail(rules, seed):
    """rules plus a duplicate of one of them (dead: the original is earlier)
    and two /25 with their /24 behind them (dead: the halves, or earlier
    rules, take its packets)."""
    import copy
    import random
    rng = random.Random(seed)
    out = list(rules)
    if rules:
        out.append(copy.deepcopy(rules[rng.randrange(len(rules))]))
    out += [_l4("h0", "172.31.7.0/25", "tcp", 0, 65535), _l4("h1", "172.31.7.128/25", "tcp", 0, 65535),
            _l4("h", "172.31.7.0/24", "tcp", 0, 65535, M.DENY)]
    return out
