"""The hop-closure tests' shared definitions (tests/test_reach_hops_cpu.py,
tests/test_gpu_reach_hops.py): hops_ref, the numpy level-synchronous
breadth-first search that defines cls_reach_hops's hop counts; sums, every
other output as a function of the hop counts; and synthetic [P, N, N] verdict
matrices over graphs no rule table would produce -- a directed path, a cycle,
two cliques joined by one bridge edge, a star, an empty and a complete graph,
seeded random graphs of out-degree about 2 -- whose edges are spread over the
probes, whose non-edges are filled with the bytes 0, 1 and 3, and whose
diagonal holds ALLOW bytes that must be ignored."""
import functools

import numpy as np

ALLOW, NONE = 2, 255
GRAPHS = ("path", "cycle", "cliques", "star", "empty", "complete", "random1", "random2")


def hops_ref(adj, H=0):
    """hops [N, N] u8 of the boolean adjacency adj[s, d] (the diagonal is
    ignored): level L holds what the frontier of level L - 1 reaches and no
    earlier level did, for L = 1 .. H (0: 254); 255 for the rest."""
    H = H or 254
    a = np.array(adj, bool)
    n = len(a)
    a[np.arange(n), np.arange(n)] = False
    af = a.astype(np.float32)
    reached = np.eye(n, dtype=bool)
    hops = np.full((n, n), NONE, np.uint8)
    hops[reached] = 0
    front = reached.copy()
    for level in range(1, H + 1):
        front = ((front.astype(np.float32) @ af) > 0) & ~reached     # (sums < 2^24: exact)
        if not front.any():
            break
        hops[front] = level
        reached |= front
    return hops


def sums(hops):
    """(reach [N] u32, exposed [N] u32, levels [256] u64, closure [N, W] u64)
    of a hops array."""
    n = len(hops)
    w = (n + 63) // 64
    got = hops != NONE
    reach = (got.sum(axis=1) - 1).astype(np.uint32)
    exposed = (got.sum(axis=0) - 1).astype(np.uint32)
    levels = np.bincount(hops.ravel(), minlength=256).astype(np.uint64)
    bits = np.zeros((n, w * 64), np.uint8)
    bits[:, :n] = got
    closure = np.ascontiguousarray(np.packbits(bits.reshape(n, w, 64), axis=2, bitorder="little")).view("<u8")
    return reach, exposed, levels, closure.reshape(n, w).astype(np.uint64)


def graph(name, n):
    """The boolean adjacency [n, n] of a named graph (n >= 1)."""
    a = np.zeros((n, n), bool)
    i = np.arange(n)
    if name == "path":
        a[i[:-1], i[1:]] = True
    elif name == "cycle":
        a[i, (i + 1) % n] = True
    elif name == "cliques":
        h = (n + 1) // 2
        a[:h, :h] = True
        a[h:, h:] = True
        if h < n:
            a[h - 1, h] = True                       # the bridge, one way
    elif name == "star":
        a[0, :] = True                               # the centre reaches every leaf, odd leaves reach it
        a[1::2, 0] = True
    elif name == "complete":
        a[:] = True
    elif name.startswith("random"):
        rng = np.random.default_rng(100 * int(name[6:]) + n)
        a = rng.random((n, n)) < 2.0 / max(n, 2)
    elif name != "empty":
        raise KeyError(name)
    a[i, i] = False
    return a


@functools.lru_cache(maxsize=None)
def synthetic(name, n, p, seed=0):
    """(matrix [p, n, n] u8, adjacency): every edge is ALLOW in one to p of
    the probes, every other cell off the diagonal is 0, 1 or 3 in all of them,
    and the diagonal is ALLOW in every probe."""
    a = graph(name, n)
    rng = np.random.default_rng(seed + 7 * n + p)
    m = rng.choice(np.array([0, 1, 3], np.uint8), size=(p, n, n))
    first = rng.integers(0, p, (n, n))               # the probe that surely carries the edge
    more = rng.random((p, n, n)) < 0.3
    carries = (np.arange(p)[:, None, None] == first[None]) | more
    m[carries & a[None]] = ALLOW
    m[:, np.arange(n), np.arange(n)] = ALLOW
    assert (((m == ALLOW).any(axis=0) & ~np.eye(n, dtype=bool)) == a).all()
    m.setflags(write=False)
    a.setflags(write=False)
    return m, a


@functools.lru_cache(maxsize=None)
def synthetic_ref(name, n, H=0):
    """hops_ref of a named graph, and its sums; shared and never modified."""
    hops = hops_ref(graph(name, n), H)
    out = (hops,) + sums(hops)
    for x in out:
        x.setflags(write=False)
    return out


def adjacency(want):
    """The graph of a [P, N, N] verdict matrix: ALLOW under some probe."""
    return (np.asarray(want) == ALLOW).any(axis=0)
