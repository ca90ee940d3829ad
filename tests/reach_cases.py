"""The reachability-matrix tests' shared case (tests/test_gpu_reach.py): a
rendered global table and 12 random local ACLs over 24 interfaces
(test_gpu_connect_scale.build), 37 endpoints drawn with repeats from all the
interfaces -- several on one interface, some on the global ACL's if0..if2,
one on an interface without an ACL -- with addresses mixed from the global
table's pod IPs and the local prefix pool (both families for the 16-byte
layout), and three probes: TCP and UDP on table ports and protocol 47.  The
expected matrix is the C oracle's (orc_test_connection_hits) over the
expanded rows, computed once per family and never modified."""
import functools

import numpy as np

N_EP, N_LOCAL, N_IF, CFG = 37, 12, 24, 2
# seeds whose oracle matrix has >= 3 distinct ConnectionActions and allow rows
# that are neither all zero nor all full (asserted in case())
SEEDS = {4: 1, 16: 1}
ALLOW = 2


class _NoEngine:
    """build() only installs ACLs: the oracle needs none."""

    def acl_put(self, *a):
        return 0


def endpoints(seed, fam, bind, ifs, pool, spec, n=N_EP):
    """(interface index per endpoint, addresses)."""
    from test_gpu_connect_scale import traffic
    rng = np.random.default_rng(1000 + seed)
    at = rng.integers(0, len(ifs), n)
    free = [i for i, name in enumerate(ifs) if bind[name] == [None, None]]
    assert free, "no interface without an ACL"
    fixed = [0, 1, 2, free[0], free[0]][:n]           # the global ACL's interfaces, one unbound (twice)
    at[:len(fixed)] = fixed
    addrs = traffic(seed, n, pool, spec, fam)["src"]
    return at, addrs


def probes(spec):
    """(proto, sport, dport) x 3: TCP and UDP on table ports, protocol 47."""
    tp = int(spec["ports"][0])
    return np.array([0, 1, 47], np.uint8), np.array([40000, 53000, 0], np.uint16), np.array([tp, 53, 0], np.uint16)


def expand(at, addrs, pr, sp, dp):
    """The matrix's rows as a connection batch: cell (p, s, d) at (p N + s) N + d."""
    n, p = len(at), len(pr)
    pi, si, di = np.meshgrid(np.arange(p), np.arange(n), np.arange(n), indexing="ij")
    pi, si, di = pi.ravel(), si.ravel(), di.ravel()
    tr = {"src": addrs[si], "dst": addrs[di], "proto": pr[pi], "sport": sp[pi], "dport": dp[pi]}
    return at[si], at[di], tr


@functools.lru_cache(maxsize=None)
def case(fam, seed=None, n=N_EP):
    """The case of a family: ACLs, endpoints, probes and the oracle's matrix
    with its per-ACL counters."""
    from test_gpu_connect_scale import build, oracle_connections
    seed = SEEDS[fam] if seed is None else seed
    ifs, bind, by_name, pool, spec = build(_NoEngine(), seed, n_local=N_LOCAL, n_if=N_IF, cfg=CFG, fam=fam)
    at, addrs = endpoints(seed, fam, bind, ifs, pool, spec, n)
    pr, sp, dp = probes(spec)
    si, di, tr = expand(at, addrs, pr, sp, dp)
    want, counts = oracle_connections(bind, by_name, ifs, si, di, tr, fam)
    want = want.reshape(len(pr), n, n)
    want.setflags(write=False)
    return dict(seed=seed, fam=fam, ifs=ifs, bind=bind, by_name=by_name, at=at, addrs=addrs, pr=pr, sp=sp, dp=dp,
                si=si, di=di, tr=tr, want=want, counts=counts)


def diverse(want) -> bool:
    """>= 3 distinct ConnectionActions; allow rows both non-zero and non-full."""
    allow = (want == ALLOW).sum(axis=2)
    return len(np.unique(want)) >= 3 and bool((allow > 0).any()) and bool((allow < want.shape[2]).any())


def install(eng, c):
    """The case's ACLs on an engine; the endpoints' interface ids."""
    from test_gpu_connect_scale import build
    build(eng, c["seed"], n_local=N_LOCAL, n_if=N_IF, cfg=CFG, fam=c["fam"])
    return install_ids(eng, c)


def install_ids(eng, c):
    """The endpoints' interface ids on an engine that has the case's ACLs."""
    return np.array([eng.if_id(x) for x in c["ifs"]], np.uint32)[c["at"]]
