"""The port sweep tests' shared helpers (tests/test_gpu_reach_ports.py,
tests/test_reach_ports_cpu.py): ranges_ref, the numpy definition of what
cls_reach_ports reports of a [n, n, ports] verdict array; class_starts, an
independent restatement of the port class starts from model.Rule objects;
oracle_at, the OpenMP oracle (oracle.connect_fast, pinned to the literal one by
test_oracle_pin_cpu.py) over endpoints x ports of a reach_cases case; brute,
six endpoints of reach_cases.case(fam) x all 65,536 ports, computed once per
(family, protocol) and never modified."""
import functools

import numpy as np

import reach_cases as rc

SPORT = {0: 40000, 1: 53000, 2: 0, 47: 0}
N_BRUTE = 6


def ranges_ref(v, starts=None, cap=None):
    """(records, total, runs [n, n] u32, allow_ports [n, n] u32, hist [4] u64)
    of v [n, n, 65536] u8 -- or v [n, n, K] with the K ascending class starts
    (starts[0] == 0; class k is starts[k] .. starts[k + 1] - 1, the last one
    ends at 65535).  records: the maximal ranges in (src, dst, port_lo)
    order, the first cap of them."""
    from vpp_amd import _abi
    v = np.asarray(v, np.uint8)
    n, w = v.shape[0], v.shape[2]
    starts = np.arange(65536, dtype=np.int64) if starts is None else np.asarray(starts, np.int64)
    assert v.shape[:2] == (n, n) and len(starts) == w and starts[0] == 0 and (np.diff(starts) > 0).all()
    width = np.diff(np.append(starts, 65536))
    flat = v.reshape(n * n, w)
    first = np.ones(flat.shape, bool)
    first[:, 1:] = flat[:, 1:] != flat[:, :-1]
    pair, k = np.nonzero(first)                       # row-major: (pair, class) ascending
    rec = np.zeros(len(pair), _abi.PORT_RANGE)
    rec["src"], rec["dst"], rec["port_lo"], rec["action"] = pair // n, pair % n, starts[k], flat[pair, k]
    # a range ends before the next start of its pair, or at 65535
    nxt = np.append(starts[k[1:]] - 1, 65535)
    last = np.append(pair[1:] != pair[:-1], True)
    rec["port_hi"] = np.where(last, 65535, nxt)
    runs = first.sum(axis=1).astype(np.uint32).reshape(n, n)
    allow = ((flat == rc.ALLOW) * width[None, :]).sum(axis=1).astype(np.uint32).reshape(n, n)
    hist = np.array([((flat == a) * width[None, :]).sum() for a in range(4)], np.uint64)
    return rec[:len(rec) if cap is None else cap], len(rec), runs, allow, hist


def class_starts(rule_lists, proto):
    """The sorted union of the class starts of model.Rule lists for proto: 0,
    and lo16 and hi16 + 1 <= 65535 of every rule with a TCP (0) / UDP (1)
    destination range that is not reversed after the u16 truncation."""
    s = {0}
    for rules in rule_lists:
        for r in rules:
            ipr = r.matches.ip_rule if r.matches is not None else None
            l4 = None if ipr is None or proto > 1 else (ipr.tcp, ipr.udp)[proto]
            rng = l4.destination_port_range if l4 is not None else None
            if rng is None:
                continue
            lo, hi = rng.lower_port & 0xFFFF, rng.upper_port & 0xFFFF
            if lo <= hi:
                s.add(lo)
                if hi < 65535:
                    s.add(hi + 1)
    return np.array(sorted(s), np.int64)


def allowed_starts(rules, proto):
    """Every value cls_port_classes may return for one rule list: 0, lo16 and
    hi16 + 1 <= 65535 of the rules with a destination range for proto (the
    reversed ones too); and the (lo16, hi16) pairs themselves."""
    ok, pairs = {0}, []
    for r in rules:
        ipr = r.matches.ip_rule if r.matches is not None else None
        l4 = None if ipr is None or proto > 1 else (ipr.tcp, ipr.udp)[proto]
        rng = l4.destination_port_range if l4 is not None else None
        if rng is None:
            continue
        lo, hi = rng.lower_port & 0xFFFF, rng.upper_port & 0xFFFF
        pairs.append((lo, hi))
        ok.add(lo)
        if hi < 65535:
            ok.add(hi + 1)
    return ok, pairs


def bound_rules(c, eps):
    """The rule lists of the ACLs bound to the interfaces of endpoints eps."""
    names = set()
    for i in np.unique(c["at"][eps]):
        names.update(x for x in c["bind"][c["ifs"][i]] if x is not None)
    return [c["by_name"][x] for x in sorted(names)]


@functools.lru_cache(maxsize=None)
def _tables(fam, changed):
    import oracle
    import reach_diff_cases as dc
    c = dc.after(fam) if changed else rc.case(fam)
    names = sorted(c["by_name"])
    tabs = [oracle.FastTable(oracle.rules_to_c(c["by_name"][x])) for x in names]
    if_in = [names.index(c["bind"][f][0]) if c["bind"][f][0] else -1 for f in c["ifs"]]
    if_out = [names.index(c["bind"][f][1]) if c["bind"][f][1] else -1 for f in c["ifs"]]
    return c, tabs, if_in, if_out


def oracle_at(fam, eps, proto, ports, changed=False, pairs=None):
    """The oracle's ConnectionAction [len(eps), len(eps), len(ports)] of the
    case's endpoints eps at destination ports `ports` (source port
    SPORT[proto]); with pairs = (s, d, port) index arrays, those cells only."""
    import oracle
    c, tabs, if_in, if_out = _tables(fam, changed)
    eps, ports = np.asarray(eps), np.asarray(ports)
    if pairs is None:
        s, d, p = (x.ravel() for x in np.meshgrid(np.arange(len(eps)), np.arange(len(eps)), np.arange(len(ports)),
                                                  indexing="ij"))
        dport = ports[p]
    else:
        s, d, dport = pairs
    m = len(s)
    tr = {"src": c["addrs"][eps[s]], "dst": c["addrs"][eps[d]], "proto": np.full(m, proto, np.uint8),
          "sport": np.full(m, SPORT[proto], np.uint16), "dport": dport.astype(np.uint16)}
    out = oracle.connect_fast(tabs, if_in, if_out, c["at"][eps[s]], c["at"][eps[d]], tr, af=fam)
    return out if pairs is not None else out.reshape(len(eps), len(eps), len(ports))


@functools.lru_cache(maxsize=None)
def brute_endpoints(fam, proto):
    """Six endpoints of the case on interfaces that do not bind `global` (the
    brute force over a global-table endpoint takes many times longer), chosen
    greedily at the class starts: each step adds the endpoint that brings the
    most ranges -- and, first, the most distinct ConnectionActions -- to the
    pairs among the chosen."""
    c = rc.case(fam)
    free = [e for e in range(rc.N_EP) if "global" not in c["bind"][c["ifs"][c["at"][e]]]]
    starts = class_starts(bound_rules(c, free), proto)
    v = oracle_at(fam, free, proto, starts)
    change = np.ones(v.shape, bool)
    change[:, :, 1:] = v[:, :, 1:] != v[:, :, :-1]
    runs = change.sum(axis=2)

    def score(sel):
        sub = v[np.ix_(sel, sel)]
        return len(np.unique(sub)), int(runs[np.ix_(sel, sel)].sum())

    sel = []
    while len(sel) < N_BRUTE:
        sel.append(max((e for e in range(len(free)) if e not in sel), key=lambda e: score(sel + [e]) + (-e,)))
    return tuple(free[e] for e in sorted(sel))


@functools.lru_cache(maxsize=None)
def brute(fam, proto):
    """(endpoints, verdicts [6, 6, 65536] u8, read-only): every port through
    the oracle."""
    eps = brute_endpoints(fam, proto)
    v = oracle_at(fam, eps, proto, np.arange(65536))
    v.setflags(write=False)
    return np.array(eps), v


def lookup(rec, n, s, d, port):
    """The action of the ranges rec (complete, in order) at cells (s, d, port)."""
    key = (rec["src"].astype(np.int64) * n + rec["dst"]) * 65536 + rec["port_lo"]
    at = np.searchsorted(key, (np.asarray(s, np.int64) * n + d) * 65536 + port, side="right") - 1
    r = rec[at]
    assert ((r["src"] == s) & (r["dst"] == d) & (r["port_lo"] <= port) & (port <= r["port_hi"])).all()
    return r["action"]
