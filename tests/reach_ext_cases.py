"""The external sweep tests' shared helpers (tests/test_gpu_reach_ext.py,
tests/test_reach_ext_cpu.py): class_starts, an independent restatement of the
IPv4 address class starts from model.Rule objects (vpp_amd.gonet's ParseCIDR
and networkNumberAndMask; only 4-byte network numbers count); ranges_ref, the
numpy definition of what cls_reach_external reports of a [D, P, N, K] verdict
array; oracle_at, the OpenMP oracle (oracle.connect_fast, pinned to the
literal one by test_oracle_pin_cpu.py) over directions x probes x endpoints x
remote addresses of a reach_cases case, the remote interface being `if0`
(bound to the global table both ways); lookup, the action of a line's ranges
at an address."""
import functools

import numpy as np

import reach_cases as rc

EXT_IF = "if0"
ALL32 = 1 << 32
DIRS = {"egress": 0, "ingress": 1}


def net_interval(cidr):
    """(lo, hi) of the IPv4 addresses the network string contains, or None:
    a string net.ParseCIDR refuses, or a network whose number
    (networkNumberAndMask) is not 4 bytes, contains none."""
    from vpp_amd import gonet
    if not cidr:
        return None
    _, net = gonet.parse_cidr(cidr)
    if net is None:
        return None
    nn, m = net._network_number_and_mask()
    if nn is None or len(nn) != 4:
        return None
    mask = int.from_bytes(m, "big")
    lo = int.from_bytes(nn, "big") & mask
    return lo, lo | (~mask & 0xFFFFFFFF)


def rule_networks(rules):
    """The source and destination network strings of model.Rule objects."""
    for r in rules:
        ipr = r.matches.ip_rule if r.matches is not None else None
        ip = ipr.ip if ipr is not None else None
        if ip is not None:
            yield ip.source_network
            yield ip.destination_network


def allowed_starts(rules):
    """Every value cls_addr_classes may return for one rule list, and the
    (lo, hi) intervals themselves."""
    ok, ivs = {0}, []
    for s in rule_networks(rules):
        iv = net_interval(s)
        if iv is not None:
            ivs.append(iv)
            ok.add(iv[0])
            if iv[1] < 0xFFFFFFFF:
                ok.add(iv[1] + 1)
    return ok, ivs


def class_starts(rule_lists):
    """The sorted union of the class starts of model.Rule lists: 0, and lo and
    hi + 1 <= 2^32 - 1 of every network that holds IPv4 addresses."""
    s = {0}
    for rules in rule_lists:
        s |= allowed_starts(rules)[0]
    return np.array(sorted(s), np.int64)


def bound_rules(c, eps, ext=EXT_IF):
    """The rule lists of the ACLs bound to the interfaces of endpoints eps and
    to the remote interface."""
    names = set(x for x in c["bind"][ext] if x is not None)
    for i in np.unique(c["at"][np.asarray(eps)]):
        names.update(x for x in c["bind"][c["ifs"][i]] if x is not None)
    return [c["by_name"][x] for x in sorted(names)]


def ranges_ref(v, starts, cap=None, dirs=None):
    """(records, total, runs [D, P, N] u32, allow_addrs [D, P, N] u64, hist
    [D, P, 4] u64) of v [D, P, N, K] u8 at the K ascending class starts
    (starts[0] == 0; class k is starts[k] .. starts[k + 1] - 1, the last one
    ends at 2^32 - 1).  records: the maximal ranges in (dir, probe, src,
    addr_lo) order, the first cap of them; dirs: the direction (0 egress, 1
    ingress) of each of the D indices (default 0 .. D - 1)."""
    from vpp_amd import _abi
    v = np.asarray(v, np.uint8)
    nd, p, n, w = v.shape
    dirs = np.arange(nd) if dirs is None else np.asarray(dirs)
    starts = np.asarray(starts, np.int64)
    assert len(dirs) == nd and len(starts) == w and starts[0] == 0 and (np.diff(starts) > 0).all()
    assert starts[-1] < ALL32
    width = np.diff(np.append(starts, ALL32)).astype(np.uint64)
    flat = v.reshape(nd * p * n, w)
    first = np.ones(flat.shape, bool)
    first[:, 1:] = flat[:, 1:] != flat[:, :-1]
    line, k = np.nonzero(first)                       # row-major: (line, class) ascending
    rec = np.zeros(len(line), _abi.ADDR_RANGE)
    rec["dir"], rec["probe"], rec["src"] = dirs[line // (p * n)], line // n % p, line % n
    rec["addr_lo"], rec["action"] = starts[k], flat[line, k]
    # a range ends before the next start of its line, or at 2^32 - 1
    nxt = np.append(starts[k[1:]] - 1, ALL32 - 1)
    last = np.append(line[1:] != line[:-1], True)
    rec["addr_hi"] = np.where(last, ALL32 - 1, nxt)
    runs = first.sum(axis=1).astype(np.uint32).reshape(nd, p, n)
    allow = ((flat == rc.ALLOW) * width[None, :]).sum(axis=1, dtype=np.uint64).reshape(nd, p, n)
    hist = np.stack([((flat == a) * width[None, :]).sum(axis=1, dtype=np.uint64).reshape(nd, p, n).sum(
        axis=2, dtype=np.uint64) for a in range(4)], axis=2)
    return rec[:len(rec) if cap is None else cap], len(rec), runs, allow, hist


def mapped(addrs):
    """::ffff:a as (n, 16) network-order bytes."""
    a = np.asarray(addrs, np.int64)
    out = np.zeros((len(a), 16), np.uint8)
    out[:, 10:12] = 0xFF
    out[:, 12:] = a.astype(">u4").view(np.uint8).reshape(-1, 4)
    return out


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


def tables_with(fam, rules, if_name, outbound=True):
    """The case's oracle tables with one more ACL bound to interface if_name
    (outbound: toward the interface's pods), for oracle_cells / oracle_at."""
    import oracle
    c, tabs, if_in, if_out = _tables(fam, False)
    tabs, if_in, if_out = tabs + [oracle.FastTable(oracle.rules_to_c(rules))], list(if_in), list(if_out)
    (if_out if outbound else if_in)[c["ifs"].index(if_name)] = len(tabs) - 1
    return c, tabs, if_in, if_out


def oracle_cells(fam, d, p, s, addr, changed=False, ext=EXT_IF, tables=None):
    """The oracle's ConnectionAction of single cells: direction d (0 egress,
    1 ingress), probe p, endpoint s of the case and remote address addr, as
    index arrays of one length; tables: tables_with's, instead of the case's."""
    import oracle
    c, tabs, if_in, if_out = tables or _tables(fam, changed)
    d, p, s = np.asarray(d), np.asarray(p), np.asarray(s)
    ext_at = np.full(len(s), c["ifs"].index(ext))
    pod_at, pod = c["at"][s], c["addrs"][s]
    rem = mapped(addr) if fam == 16 else np.asarray(addr, np.int64).astype(np.uint32)
    ing = d == 1
    sel = ing[:, None] if fam == 16 else ing
    tr = {"src": np.where(sel, rem, pod), "dst": np.where(sel, pod, rem), "proto": c["pr"][p], "sport": c["sp"][p],
          "dport": c["dp"][p]}
    return oracle.connect_fast(tabs, if_in, if_out, np.where(ing, ext_at, pod_at), np.where(ing, pod_at, ext_at), tr,
                               af=fam)


def oracle_at(fam, dirs, eps, addrs, changed=False, ext=EXT_IF, tables=None):
    """The oracle's ConnectionAction [len(dirs), P, len(eps), len(addrs)] of
    the case's endpoints eps at remote addresses addrs through `ext`; dirs:
    directions (0 egress: pod -> address, 1 ingress: address -> pod)."""
    c = rc.case(fam)
    dirs, eps, addrs = np.asarray(dirs), np.asarray(eps), np.asarray(addrs, np.int64)
    di, pi, si, ai = (x.ravel() for x in np.meshgrid(np.arange(len(dirs)), np.arange(len(c["pr"])),
                                                     np.arange(len(eps)), np.arange(len(addrs)), indexing="ij"))
    v = oracle_cells(fam, dirs[di], pi, eps[si], addrs[ai], changed, ext, tables)
    return v.reshape(len(dirs), len(c["pr"]), len(eps), len(addrs))


def line_of(rec, p=3, n=rc.N_EP, nd=2):
    """The line number (d P + p) N + s of every record (d: the direction's
    index among nd directions in ascending order -- with nd == 1 it is 0)."""
    d = rec["dir"].astype(np.int64) if nd == 2 else np.zeros(len(rec), np.int64)
    return (d * p + rec["probe"]) * n + rec["src"]


def lookup(rec, line, addr, p=3, n=rc.N_EP, nd=2):
    """The action of the ranges rec (complete, in order) at address addr of
    line `line` (arrays of one length)."""
    key = line_of(rec, p, n, nd) * ALL32 + rec["addr_lo"]
    line, addr = np.asarray(line, np.int64), np.asarray(addr, np.int64)
    at = np.searchsorted(key, line * ALL32 + addr, side="right") - 1
    r = rec[at]
    assert ((line_of(r, p, n, nd) == line) & (r["addr_lo"] <= addr) & (addr <= r["addr_hi"])).all()
    return r["action"]
