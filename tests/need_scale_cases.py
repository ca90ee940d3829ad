"""The rule necessity sweep at the sizes where its waves loop: the shared
helpers of tests/test_need_scale_cpu.py and tests/test_gpu_table_need_scale.py.

table, the seeded generator: n_src consecutive /24 source networks, n_dst /24
destination networks and n_ranges disjoint port ranges with gaps between them.
About 93 % of the rules are narrow (/24 to /24; four in five of those take
every port of TCP or UDP, the rest one range), about 5 % use the /20 around
both /24 and about 2 % the /16, always with one port range; PERMIT and DENY
in random order.  Broad all-port rules would give every cell an early first
match and leave the rules behind them dead: with this mixture rules stay first
matches through every stride of 4,096 rules.

The references, in order of independence: Engine.table_need_host (the same
definition in plain serial C++, pinned to the oracle on small tables by
test_table_need_cpu.py), computed once per shape and shared (host); and
literal_for_rule, written from the Python rule fields alone
(cover_cases.net_interval and the port ranges, none of the library's code) for
a narrow rule, whose cells all lie in one (source class, destination class)
pair."""
import numpy as np

import cover_cases as cc
from reach_ext_cases import net_interval
from vpp_amd import model as M

SKIPPED, DEAD, REDUNDANT, NEEDED = 0, 1, 2, 3
LDS_TWO_PER_CU, LDS_MAX = 80 * 1024, 144 * 1024       # k_need.hip: launch_cells' per_cu threshold, kColsLdsMax
CELLS_WAVES = 16                                      # kCellsWaves: waves (pairs) of one need_cells workgroup
STRIDE = 4096                                         # rules per stride: 64 lanes x 64 bits
FOLD_STEP_CELLS = 2 * 16 * 256                        # cover_fold: 2 workgroups per CU x 16 waves x 256 cells a step
SRC0, DST0 = 10 << 24, 172 << 24 | 16 << 16           # 10.0.0.0, 172.16.0.0

# name: (rules, n_src, n_dst, port ranges, seed, a TCP-only range from port 0).  R, W, form and the column rows T W 8:
SHAPES = {
    "a": (1000, 280, 256, 6, 4, False),        # W 16, NW 1, a few KiB; 9 passes of the pair loop
    "b": (4096, 150, 130, 20, 2, False),       # W 64, NW 1 with the last word full, 42 KiB
    "c": (4097, 150, 130, 20, 304, False),     # W 65, NW 2 with one word in the second register: the seed makes
    "c_odd": (4097, 150, 130, 20, 304, True),  # rule 4096 a /16 (a first and a second match); c_odd: W 65, odd T
    "d": (8100, 120, 100, 34, 4, False),       # W 127, NW 2, 138.9 KiB: one workgroup per CU
    "e": (12000, 120, 100, 16, 5, False),      # W 188, NW 4 with three live registers
    "f": (16000, 120, 100, 16, 6, False),      # W 250, NW 4 with four live registers
    "g": (16450, 140, 110, 16, 7, False),      # W 258, NW 0, 137.1 KiB: the rows in LDS, one workgroup per CU
    "h": (16450, 120, 100, 36, 8, False),      # W 258, NW 0, 298 KiB: above kColsLdsMax with no option set
    "fold": (1000, 280, 256, 18, 4, False),    # shape a with T 76: above two cover_fold steps per wave
}
MAIN = ("a", "b", "c", "d", "e", "f", "g", "h")


def _net(base, i, prefix):
    a = (base + (i << 8)) & (0xFFFFFFFF << (32 - prefix))
    return "%d.%d.%d.%d/%d" % (a >> 24, a >> 16 & 255, a >> 8 & 255, a & 255, prefix)


def port_ranges(n):
    """n disjoint ranges of 100 ports with gaps of 100, from port 1000 on."""
    return [(1000 + 200 * k, 1099 + 200 * k) for k in range(n)]


def table(r, n_src, n_dst, n_ranges, seed, tcp_zero=False):
    """The rule list (see the module docstring).  tcp_zero: TCP rules also draw
    the range 0 .. 499, which adds a single class start (500): T is odd."""
    rng = np.random.default_rng(seed)
    ranges = port_ranges(n_ranges)
    kind, s, d = rng.random(r), rng.integers(0, n_src, r), rng.integers(0, n_dst, r)
    udp, deny, allp = rng.random(r) < 0.5, rng.random(r) < 0.5, rng.random(r) < 0.8
    pick = rng.integers(0, n_ranges + 1, r)
    rules = []
    for i in range(r):
        prefix = 24 if kind[i] < 0.93 else 20 if kind[i] < 0.98 else 16
        own = ranges if udp[i] or not tcp_zero else ranges + [(0, 499)]
        lo, hi = (0, 65535) if prefix == 24 and allp[i] else own[pick[i] % len(own)]
        rules.append(cc._l4("r%d" % i, _net(SRC0, int(s[i]), prefix), "udp" if udp[i] else "tcp", lo, hi,
                            M.DENY if deny[i] else M.PERMIT, dst=_net(DST0, int(d[i]), prefix)))
    return rules


_MADE = {}


def shape(name):
    """SHAPES[name]'s rule list, made once and shared; never modified."""
    if name not in _MADE:
        _MADE[name] = table(*SHAPES[name])
    return _MADE[name]


_HOST = {}


def host(name, skip=None, key=None):
    """Engine.table_need_host of a shape, computed once per (name, key) and
    shared; never modified.  ``key`` names the skip set."""
    from vpp_amd.engine import Engine
    k = (name, key)
    assert (skip is None) == (key is None)
    if k not in _HOST:
        _HOST[k] = Engine.table_need_host(shape(name), skip=skip)
    return _HOST[k]


def skip_third(name):
    """A seeded random third of the shape's rules, the last rule never among
    them: every word of the kept row keeps a bit, and every full word loses one."""
    r = len(shape(name))
    gone = np.flatnonzero(np.random.default_rng(r).random(r - 1) < 1 / 3)
    words = np.bincount(gone >> 6, minlength=(r + 63) // 64)
    assert words[:r // 64].min() > 0 and np.all(words < np.bincount(np.arange(r) >> 6))
    return gone.tolist()


def geometry(want, r):
    """(T, W, pairs, cells, bytes of the column rows) from a result's dims."""
    ks, kd, kt, ku = want["dims"]
    t, w = kt + ku + 2, max(1, (r + 63) // 64)
    return t, w, ks * kd, ks * kd * t, t * w * 8


def cells_waves(pairs, n_cu, col_bytes, lds=True):
    """The waves launch_cells starts for a tile of ``pairs`` pairs: workgroups
    of 16, two per CU, one where the column rows in LDS are above 80 KiB."""
    lds = lds and col_bytes <= LDS_MAX
    per_cu = 1 if lds and col_bytes > LDS_TWO_PER_CU else 2
    return min((pairs + CELLS_WAVES - 1) // CELLS_WAVES, max(1, n_cu) * per_cu) * CELLS_WAVES


def tiles(pairs, t, cover_tile):
    """(pairs per tile, tiles, pairs of the last tile) of need_pass."""
    per = max(1, cover_tile // t)
    n = (pairs + per - 1) // per
    return per, n, pairs - (n - 1) * per


def cells(rules):
    """cover_cases.cells without its ceiling of 2^22 cells."""
    slo, dlo = cc.side_starts(rules, 0), cc.side_starts(rules, 1)
    proto, dport, _, _ = cc.columns(rules)
    ks, kd, t = len(slo), len(dlo), len(proto)
    return dict(src=np.repeat(slo, kd * t).astype(np.uint32), dst=np.tile(np.repeat(dlo, t), ks).astype(np.uint32),
                proto=np.tile(proto, ks * kd), dport=np.tile(dport, ks * kd))


# ---- the check from the rule fields alone ---------------------------------------------

_FIELDS = {}


def fields(rules):
    """The rules as arrays, from the model.Rule fields: source and destination
    interval, protocol (0 TCP, 1 UDP), destination port range, action."""
    if id(rules) not in _FIELDS:
        out = np.zeros((len(rules), 8), np.int64)
        for k, r in enumerate(rules):
            ipr = r.matches.ip_rule
            l4 = ipr.tcp if ipr.tcp is not None else ipr.udp
            assert (ipr.tcp is None) != (ipr.udp is None) and ipr.icmp is None and ipr.other is None
            src, rng = l4.source_port_range, l4.destination_port_range
            assert (src.lower_port, src.upper_port) == (0, 65535) and 0 <= rng.lower_port <= rng.upper_port <= 65535
            out[k] = (*net_interval(ipr.ip.source_network), *net_interval(ipr.ip.destination_network),
                      0 if ipr.tcp is not None else 1, rng.lower_port, rng.upper_port, r.actions.acl_action)
        _FIELDS[id(rules)] = (rules, out)
    return _FIELDS[id(rules)][1]


def narrow(rules):
    """The indices of the /24 to /24 rules."""
    f = fields(rules)
    return np.flatnonzero((f[:, 1] - f[:, 0] == 255) & (f[:, 3] - f[:, 2] == 255))


def literal_for_rule(rules, r):
    """What the sweep reports of the narrow rule r, evalACL taken literally
    over the T columns of r's one (source class, destination class) pair: a
    rule whose networks contain the pair takes a TCP (UDP) column when it is a
    TCP (UDP) rule and the column's port lies in its range, no ICMP column, and
    the column of the protocols above 2 whatever its section says.  Returns
    (first[r], changed[r], need[r], witness[r] as a tuple)."""
    f = fields(rules)
    s_lo, s_hi, d_lo, d_hi = f[r, :4]
    assert s_hi - s_lo == 255 and d_hi - d_lo == 255
    # every network is aligned and at least a /24: the /24 is one class on each side, starting at its own start
    at = np.flatnonzero((f[:, 0] <= s_lo) & (s_hi <= f[:, 1]) & (f[:, 2] <= d_lo) & (d_hi <= f[:, 3]))
    proto, dport, _, _ = cc.columns(rules)
    proto, dport = proto.astype(np.int64)[None, :], dport.astype(np.int64)[None, :]
    g = f[at]
    hit = (proto == 3) | ((proto == g[:, 4:5]) & (g[:, 5:6] <= dport) & (dport <= g[:, 6:7]))     # [rules of the pair, T]
    n, act = len(rules), np.concatenate([f[:, 7], [M.DENY]])
    order = np.cumsum(hit, axis=0)
    first = np.where(order.max(axis=0) >= 1, at[np.argmax(order == 1, axis=0)], n)
    second = np.where(order.max(axis=0) >= 2, at[np.argmax(order == 2, axis=0)], n)
    mine = first == r
    chg = np.flatnonzero(mine & (act[first] != act[second]))
    need = DEAD if not mine.any() else NEEDED if len(chg) else REDUNDANT
    wit = (0, 0, 0, 0, 0, 0)
    if len(chg):
        j = chg[0]
        wit = (int(s_lo), int(d_lo), int(dport[0, j]), int(proto[0, j]), 0x80 | int(act[second[j]]), int(second[j]))
    return int(mine.sum()), len(chg), need, wit


def sample(rules, want, total=64):
    """``total`` narrow rules (seeded), taken from the strides in turn and
    within a stride in turn from its DEAD, REDUNDANT and NEEDED ones."""
    r = len(rules)
    nar = narrow(rules)
    rng = np.random.default_rng(r)
    queues = []
    for k in range((r + STRIDE - 1) // STRIDE):
        mine = nar[nar >> 12 == k]
        by = [rng.permutation(mine[want["need"][mine] == v]).tolist() for v in (DEAD, REDUNDANT, NEEDED)]
        queues.append([x for i in range(max(map(len, by), default=0)) for b in by for x in b[i:i + 1]])
    out = []
    while len(out) < total and any(queues):
        for q in queues:
            if q and len(out) < total:
                out.append(q.pop(0))
    return sorted(out)
