"""Batch sizes, rule lists and traffic that put a classify launch in a chosen
loop at a chosen search depth (test infrastructure; plain Python, no GPU).

classify4_cls (vpp_amd/csrc/kernels_dev.hpp) has three loops: full grid steps
(``g < nfull``, ``nfull = nsteps / nthreads * nthreads`` groups of four packets:
the only loop that takes the depth-specialised ``kD``, the ordered loads and
the cached protocol load), leftover groups of four (``kD = -1``), and a
per-packet tail.  cls_grid (engine.cpp) launches ``min(n_cu * per_cu,
ceil(n / 4096))`` workgroups of 1024 threads, so below saturation a batch
reaches the full-step loop only when ``n`` is a multiple of 4096.  ``census4``
/ ``census16`` compute, for a batch size, what each loop gets; the tests
assert it before they rely on it.

The rule lists are built without randomness, so the depth each declares
(header ``bv_steps_d``: the number of probes of the destination search in
list modes 3 and 4) does not drift: a "ladder" of ``m`` disjoint destination
/24s has ``2 m + 1`` destination intervals per candidate list, depth
``ceil(log2(2 m + 1))``.
"""
from __future__ import annotations

import numpy as np

from vpp_amd import model as M

BLOCK = 1024          # kClsBlock
GROUP = 4             # packets per lane per step
WAVE_STEP = 256       # classify16_cls: packets per wave-step


def per_cu(lds_resident, wg_per_cu=0):
    """Workgroups per CU of a classifier launch (engine.cpp cls_grid)."""
    by_threads = 2048 // BLOCK
    p = 1 if lds_resident else by_threads
    if wg_per_cu > 0:
        p = max(1, min(by_threads, wg_per_cu))
    return p


def grid_of(n, n_cu, lds_resident, wg_per_cu=0, block=BLOCK):
    want = (n + GROUP * block - 1) // (GROUP * block)
    return max(1, min(n_cu * per_cu(lds_resident, wg_per_cu), want))


def census4(n, n_cu, lds_resident, wg_per_cu=0, block=BLOCK):
    """(grid, rounds, leftover_groups, tail) of a vector classify4_cls launch
    over n packets: ``rounds`` full grid steps per lane, the groups of four
    the leftover loop takes, the packets the per-packet tail takes."""
    grid = grid_of(n, n_cu, lds_resident, wg_per_cu, block)
    nthreads = grid * block
    nsteps = n // GROUP
    rounds = nsteps // nthreads
    return grid, rounds, nsteps - rounds * nthreads, n - GROUP * nsteps


def census16(n, n_cu, lds_resident, wg_per_cu=0, block=BLOCK):
    """(grid, wave_steps, tail) of a classify16_cls launch: whole 256-packet
    wave-steps (every one takes the template depth), then the per-packet
    tail."""
    grid = grid_of(n, n_cu, lds_resident, wg_per_cu, block)
    return grid, n // WAVE_STEP, n % WAVE_STEP


def one_round(g, block=BLOCK):
    """A batch of g workgroups in which every packet is in the full-step
    loop: one round, no leftover group, no tail (g below n_cu * per_cu)."""
    return GROUP * block * g


def saturated(n_cu, pcu, rounds, L, r, block=BLOCK):
    """A batch of the saturated grid (n_cu * pcu workgroups): ``rounds`` full
    rounds, L leftover groups and r tail packets in one launch."""
    assert 0 < L < block * n_cu * pcu and 0 < r < GROUP
    return GROUP * block * n_cu * pcu * rounds + GROUP * L + r


def simulate4(n, grid, block=BLOCK):
    """The three loops of classify4_cls<kVec = true>, literally, thread by
    thread: per loop the packets it classifies (sorted)."""
    nthreads = grid * block
    nsteps = n // GROUP
    nfull = nsteps // nthreads * nthreads
    full, left, tail = [], [], []
    for tid in range(nthreads):
        g = tid
        while g < nfull:
            full.extend(range(GROUP * g, GROUP * g + GROUP))
            g += nthreads
        gi = nfull + tid
        while gi < nsteps:
            left.extend(range(GROUP * gi, GROUP * gi + GROUP))
            gi += nthreads
        i = nsteps * GROUP + tid
        while i < n:
            tail.append(i)
            i += nthreads
    return sorted(full), sorted(left), sorted(tail)


def simulate16(n, grid, block=BLOCK):
    """The two loops of classify16_cls, thread by thread: (step packets,
    tail packets), sorted."""
    nthreads = grid * block
    nsteps = n // WAVE_STEP * 64
    step, tail = [], []
    for tid in range(nthreads):
        g = tid
        while g < nsteps:
            base = 4 * (g & ~63) + (g & 63)
            step.extend(base + 64 * k for k in range(4))
            g += nthreads
        i = nsteps * 4 + tid
        while i < n:
            tail.append(i)
            i += nthreads
    return sorted(step), sorted(tail)


# batch sizes of the suite's adversarial / variant parity tests: none reaches
# the full-step loop (test_classify_steps_cpu.py)
SUITE_SIZES = {"test_gpu_parity.py": (20011, 30000, 4099, 9001),
               "test_gpu_counters.py": (40003, 65613, 70001),
               "test_gpu_rules.py": (8191, 20011),
               "test_gpu_trie_wide.py": (50000, 200000),
               "test_gpu_threads.py": (40003,)}


# ---------------------------------------------------------------------------
# rule lists for a chosen depth

ACTIONS = (M.PERMIT, M.DENY, M.REFLECT)
LADDER_PORT = 80
N_PAD = 70
RUNG0 = 20 << 24                       # 20.0.0.0: rung k is 20.0.2k.0/24
M_OF_DEPTH = {2: 1, 3: 2, 4: 5, 5: 9, 6: 17, 7: 32}     # the ladder used for each depth (32: the longest list)


def ladder_depth(m):
    """ceil(log2(2 m + 1)): the probes of a search over m rungs and the gaps around them."""
    return (2 * m).bit_length()

# source lookup -> (options, header mode, kernel source variant: 0 interval
# search, 1 hash LPM, 2 hash LPM with one length, 4 source trie)
LOOKUPS = {"hash": (dict(src_search=0, trie=0), 1, 1),
           "search": (dict(src_search=1, trie=0), 0, 0),
           "trie": (dict(src_search=1, trie=1), 4, 4),
           "host": (dict(src_search=0, trie=0), 1, 2)}


def _v4(a):
    return "%d.%d.%d.%d" % ((a >> 24) & 255, (a >> 16) & 255, (a >> 8) & 255, a & 255)


def _sources(lookup):
    """(ladder sources, padding sources) as (address, length)."""
    if lookup == "host":               # /32 only: one hashed length
        lad = [((10 << 24) | (k << 16) | 0x0507, 32) for k in (1, 2, 3)]
        pad = [((30 << 24) | (k << 16) | 0x0109, 32) for k in range(N_PAD)]
    else:
        lad = [((10 << 24) | (k << 16), 16) for k in (1, 2, 3)]
        # hash: a second hashed length among the padding, so that the table
        # keeps the several-lengths kernel
        pad = [((30 << 24) | (k << 16), 24 if (lookup == "hash" and k % 7 == 3) else 16) for k in range(N_PAD)]
    return lad, pad


class Case:
    """A rule list, the options it is compiled under, what it declares
    (header mode, list mode, depth), and the points its traffic is drawn from."""

    def __init__(self, name, rules, options, mode, list_mode, depth, variant, srcs, dsts, n_ladder):
        self.name, self.rules, self.options = name, rules, options
        self.mode, self.list_mode, self.depth, self.variant = mode, list_mode, depth, variant
        self.srcs, self.dsts, self.n_ladder = srcs, dsts, n_ladder

    def apply(self, libopt, *engines):
        for k, v in self.options.items():
            libopt.set(k, str(v), *engines)

    def __repr__(self):
        return self.name


def _points(a, ln):
    size = 1 << (32 - ln)
    return [a, a + size - 1, a + size // 2] if size > 1 else [a]


def _options(lookup, list_mode):
    o = dict(LOOKUPS[lookup][0], orient="src")
    if list_mode == 3:
        o["list_mode_max"] = 3
    return o


def ladder(m, lookup="hash", list_mode=4):
    """m disjoint destination /24s (20.0.2k.0/24, k < m; actions cycling
    PERMIT / DENY / REFLECT) under each of three sources, one TCP port, and
    N_PAD padding rules with sources of their own.  The ladder rules come
    first: rule s * m + k is source s, rung k."""
    lad, pad = _sources(lookup)
    rules = []
    for s, (a, ln) in enumerate(lad):
        for k in range(m):
            rules.append(M.l4_rule(ACTIONS[(s + k) % 3], "%s/%d" % (_v4(a), ln), "%s/24" % _v4(RUNG0 + (2 * k << 8)),
                                   "tcp", 0, 65535, LADDER_PORT, LADDER_PORT))
    for k, (a, ln) in enumerate(pad):
        rules.append(M.l4_rule(ACTIONS[k % 3], "%s/%d" % (_v4(a), ln), "", "tcp", 0, 65535, LADDER_PORT, LADDER_PORT))
    dsts = [0, 1, 0xFFFFFFFF, 0xFFFFFFFE, RUNG0 - 1, 0x80000000, 0x7FFFFFFF]
    for k in range(m):
        r = RUNG0 + (2 * k << 8)
        dsts += [r, r + 255, r + 77, r + 256, r + 511]          # the rung, the gap after it
    srcs = [p for a, ln in lad for p in _points(a, ln)]
    srcs += [p for a, ln in pad[:6] for p in _points(a, ln)]
    srcs += [0, 0xFFFFFFFF, (10 << 24) | (4 << 16), (10 << 24) | 0xFFFF, (30 << 24) | (N_PAD << 16)]
    mode, variant = LOOKUPS[lookup][1:]
    depth = ladder_depth(m)
    return Case("ladder%d_%s_%d" % (m, lookup, list_mode), rules, _options(lookup, list_mode), mode, list_mode,
                depth, variant, srcs, dsts, 3 * m)


def flat(depth, lookup="hash", list_mode=4):
    """Depth 0: N_PAD rules with distinct sources and no destination network;
    depth 1: the same with destination 128.0.0.0/1 or 0.0.0.0/1 in turn."""
    assert depth in (0, 1)
    lad, pad = _sources(lookup)
    rules = []
    for k, (a, ln) in enumerate(lad + pad):
        dst = "" if depth == 0 else ("128.0.0.0/1" if k % 2 else "0.0.0.0/1")
        rules.append(M.l4_rule(ACTIONS[k % 3], "%s/%d" % (_v4(a), ln), dst, "tcp", 0, 65535, LADDER_PORT, LADDER_PORT))
    dsts = [0, 1, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, RUNG0, 0xC0000001]
    srcs = [p for a, ln in (lad + pad) for p in _points(a, ln)[:2]]
    srcs += [0, 0xFFFFFFFF, (10 << 24) | (4 << 16), (30 << 24) | (N_PAD << 16)]
    mode, variant = LOOKUPS[lookup][1:]
    return Case("flat%d_%s_%d" % (depth, lookup, list_mode), rules, _options(lookup, list_mode), mode, list_mode,
                depth, variant, srcs, dsts, len(rules))


def for_depth(depth, lookup="hash", list_mode=4):
    if depth <= 1:
        return flat(depth, lookup, list_mode)
    return ladder(M_OF_DEPTH[depth], lookup, list_mode)


DEPTHS = (0, 1, 2, 3, 4, 5, 6, 7)


def target_rules(case):
    """The rules a batch must reach in the loop under test: every rung's rule
    under every ladder source (every rule of a flat list), and the default DENY."""
    return list(range(case.n_ladder)) + [len(case.rules)]


def ladder_traffic(case, n, seed=1, other_every=0):
    """n packets over a Case's points: a hit for every target rule, then every
    (source point, destination point) pair in turn under a cycle of
    (protocol, port) -- protocols 0 to 2 -- shuffled with a fixed seed;
    other_every = k > 0: every k-th packet of the shuffled batch gets
    protocol 47 (spread evenly over the batch, so over the loops)."""
    S = np.array(case.srcs, np.uint64).astype(np.uint32)
    D = np.array(case.dsts, np.uint64).astype(np.uint32)
    pp = np.array([(0, 80), (0, 80), (1, 80), (0, 81), (2, 80), (0, 80), (0, 79), (2, 0), (1, 0), (0, 65535),
                   (0, 80)], np.uint32)
    i = np.arange(n, dtype=np.int64)
    src = S[i % len(S)]
    dst = D[(i // len(S)) % len(D)]
    k = (i + i // (len(S) * len(D))) % len(pp)
    proto = pp[k, 0].astype(np.uint8)
    dport = pp[k, 1].astype(np.uint16)
    # a hit per ladder rule, from the rule itself
    hits = []
    for r in case.rules[:case.n_ladder]:
        ip = r.matches.ip_rule.ip
        a, ln = ip.source_network.split("/")
        q = [int(x) for x in a.split(".")]
        s0 = (q[0] << 24) | (q[1] << 16) | (q[2] << 8) | q[3]
        d0 = RUNG0 + 5
        if ip.destination_network:
            q = [int(x) for x in ip.destination_network.split("/")[0].split(".")]
            d0 = ((q[0] << 24) | (q[1] << 16) | (q[2] << 8) | q[3]) + 5
        hits.append((s0 + (3 if int(ln) < 32 else 0), d0))
    h = min(len(hits), n)
    if h:
        src[:h] = np.array([x[0] for x in hits[:h]], np.uint64).astype(np.uint32)
        dst[:h] = np.array([x[1] for x in hits[:h]], np.uint64).astype(np.uint32)
        proto[:h] = 0
        dport[:h] = LADDER_PORT
    perm = np.random.default_rng(seed).permutation(n)
    tr = dict(src=src[perm], dst=dst[perm], dport=dport[perm], proto=proto[perm])
    if other_every:
        tr["proto"][::other_every] = 47
    return tr


def reached(case, tr, upto, af=4):
    """Whether the oracle's matched-rule trace over packets [0, upto) reaches
    every target rule of the case."""
    import oracle
    _, hits = oracle.classify_hits(oracle.rules_to_c(case.rules), tr["src"], tr["dst"], tr["dport"], tr["proto"], af=af)
    return set(target_rules(case)) <= set(hits[:upto].tolist())


# (depth, lookup, list mode) of the depth tests: every depth x both sublist
# forms x the four source lookups
DEPTH_CASES = [(d, lk, lm) for lm in (4, 3) for lk in ("hash", "search", "host", "trie") for d in DEPTHS]

# the 16-byte twins (aclgen.mix_families, seed TWIN_SEED) of the depth lists
# and the depth their core image has in rep space: name -> (builder args, depth)
TWIN_SEED = 5
TWINS = {"d0": ((0,), 0), "d1": ((2,), 1), "d2": ((1,), 2), "d3": ((3,), 3), "d4": ((5,), 4), "d5": ((6,), 5),
         "d6": ((7,), 6)}


def _addr16(cidr, dflt):
    """An address inside a 16-byte rule network as a python int (IPv4 networks
    as IPv4-mapped addresses); dflt for an empty network."""
    import ipaddress
    if not cidr:
        return dflt
    net = ipaddress.ip_network(cidr, strict=False)
    a = int(net.network_address) + (5 if net.num_addresses > 5 else 0)
    return a if net.version == 6 else (0xFFFF << 32) | a


def twin(key, lookup="hash", n=0, other_every=0):
    """(case, 16-byte rules, 16-byte traffic, depth of the 16-byte core).  A
    twinned rule matches only the packets of its networks' families, so a hit
    per ladder rule is written from the 16-byte rules themselves, spread
    evenly over the whole wave-steps of the batch."""
    from aclgen import mix_families, to16
    (d,), depth = TWINS[key]
    c = for_depth(d, lookup, 4)
    rules, tr = mix_families(c.rules, ladder_traffic(c, n, other_every=other_every), TWIN_SEED)
    whole = n - n % WAVE_STEP
    if whole >= 2 * c.n_ladder:
        at = 1 + (whole // c.n_ladder) * np.arange(c.n_ladder)
        src, dst = [], []
        for r in rules[:c.n_ladder]:
            ip = r.matches.ip_rule.ip
            src.append(_addr16(ip.source_network, (0xFFFF << 32) | 1))
            dst.append(_addr16(ip.destination_network, (0xFFFF << 32) | (RUNG0 + 5)))
        tr["src"][at], tr["dst"][at] = to16(src), to16(dst)
        tr["dport"][at], tr["proto"][at] = LADDER_PORT, 0
    c = Case(c.name + "_twin", rules, c.options, c.mode, c.list_mode, c.depth, c.variant, c.srcs, c.dsts, c.n_ladder)
    return c, rules, tr, depth


# tables of the launches that go through all three loops: one per source
# lookup (depth 4), and the depth-0, depth-5 and depth-6 lists (hash LPM)
SATURATED = {"flat0": (0, "hash"), "ladder9": (5, "hash"), "ladder17": (6, "hash"),
             "search": (4, "search"), "host": (4, "host"), "trie": (4, "trie")}


def saturated_case(key, list_mode=4):
    d, lookup = SATURATED[key]
    return for_depth(d, lookup, list_mode)
