"""The reachability calls at the sizes where their kernels and host code
change path (tests/test_gpu_reach_scale.py, tests/test_reach_scale_cpu.py):
references that are exact at any N and cost index arithmetic.

testConnection is a function of the two endpoints' (interface, address) and
the probe, so the 37 endpoints of reach_cases.case(fam) serve as *kinds*: an
endpoint list in which endpoint s is of kind[s] has the matrix
want_big[p, s, d] = want[p, kind[s], kind[d]] with no oracle call of its own
(the matrix has no special diagonal: a cell with s != d of one kind equals the
small diagonal cell).  When every kind occurs m times, the histogram is m^2 x,
the allow counts are m x and the connection counters m^2 x the case's.  The
port sweep's ranges follow the kinds the same way (ports_by_kinds, from the
brute force's six endpoints).  The hop search has closed forms instead: the
hop counts of reach_hops_cases.graph's path, cycle, cliques, star, complete
and empty graphs as index arithmetic on (s, d, n) (closed_hops), a verdict
matrix that holds exactly such a graph (closed_matrix) and the other outputs
of a hops array (closed_sums), all three in torch, in row blocks, on the CPU
or a device.  Each is checked against the oracle or hops_ref where those are
affordable (tests/test_reach_scale_cpu.py)."""
import numpy as np

import reach_cases as rc

ALLOW, NONE = 2, 255
CLOSED = ("path", "cycle", "cliques", "star", "complete", "empty")
BLOCK_CELLS = 1 << 24                                    # cells per row block: int64 temporaries of 128 MB


def kinds(m, seed=0, n_kinds=rc.N_EP):
    """The kind of each of n_kinds * m endpoints: every kind m times, in a
    seeded shuffled order."""
    k = np.repeat(np.arange(n_kinds), m)
    np.random.default_rng(4000 + seed).shuffle(k)
    return k


def drawn(n, seed=0, n_kinds=rc.N_EP):
    """n kinds drawn with repeats (not uniform), every kind at least once when
    n >= n_kinds."""
    rng = np.random.default_rng(5000 + seed)
    k = rng.integers(0, n_kinds, n)
    k[rng.permutation(n)[:min(n, n_kinds)]] = np.arange(n_kinds)[:min(n, n_kinds)]
    return k


class Big(dict):
    """A case over a kind vector; want() is built on first use and kept."""

    def want(self):
        if "_want" not in self:
            k = self["kind"]
            w = np.ascontiguousarray(self["small"]["want"][:, k[:, None], k[None, :]])
            w.setflags(write=False)
            self["_want"] = w
        return self["_want"]


def by_kinds(c, kind):
    """The case c with endpoint s of kind[s]: at, addrs by kind; the probes,
    ACLs and bindings are the case's.  Sums: those of want()."""
    kind = np.asarray(kind)
    return Big(small=c, fam=c["fam"], seed=c["seed"], ifs=c["ifs"], bind=c["bind"], by_name=c["by_name"], kind=kind,
               at=c["at"][kind], addrs=c["addrs"][kind], pr=c["pr"], sp=c["sp"], dp=c["dp"], N=len(kind))


_expanded = {}


def expand(c, m, seed=0):
    """The case c with every endpoint m times (kinds(m, seed)), and the
    multiplied sums: hist [P, 4] u64, allow [P, N] u32, counts by ACL; made
    once per (case, m, seed) and shared."""
    key = (c["fam"], c["seed"], len(c["at"]), m, seed)
    if key in _expanded:
        return _expanded[key]
    b = by_kinds(c, kinds(m, seed, len(c["at"])))
    hist, allow = sums(c["want"])
    b.update(m=m, hist=hist * np.uint64(m * m), allow=(allow * np.uint32(m))[:, b["kind"]],
             counts={k: v.astype(np.uint64) * np.uint64(m * m) for k, v in c["counts"].items()})
    assert int(allow.max()) * m < 1 << 32
    _expanded[key] = b
    return b


def sums(want):
    """(hist [P, 4] u64, allow [P, N] u32) of a verdict matrix."""
    hist = np.stack([np.bincount(want[p].ravel(), minlength=4) for p in range(want.shape[0])]).astype(np.uint64)
    return hist, (want == ALLOW).sum(axis=2).astype(np.uint32)


def rows_of(b, n_probes=None):
    """The matrix's rows as a connection batch over the expanded endpoints
    (reach_cases.expand), with the probes repeated cyclically to n_probes."""
    pr, sp, dp = cyclic(b, n_probes or len(b["pr"]))
    return rc.expand(b["at"], b["addrs"], pr, sp, dp)


def cyclic(b, p):
    """The case's probes repeated cyclically to p of them."""
    i = np.arange(p) % len(b["pr"])
    return b["pr"][i], b["sp"][i], b["dp"][i]


def install_ids(eng, b):
    """The endpoints' interface ids on an engine that has the case's ACLs."""
    return np.array([eng.if_id(x) for x in b["ifs"]], np.uint32)[b["at"]]


# ---- the port sweep by kinds -------------------------------------------------

def ports_by_kinds(v, kind):
    """What reach_ports_cases.ranges_ref gives for the [N, N, 65536] array
    v[kind][:, kind] -- (records, total, runs, allow_ports, hist) -- from the
    small v [n, n, 65536] alone: pair (s, d) has the records of (kind[s],
    kind[d]) with src and dst rewritten, in (src, dst, port_lo) order."""
    import reach_ports_cases as pc
    kind = np.asarray(kind)
    n, N = v.shape[0], len(kind)
    rec, _, runs, allow, _ = pc.ranges_ref(v)
    start = np.cumsum(runs.ravel(), dtype=np.int64) - runs.ravel()        # a small pair's first record
    small = (kind[:, None] * n + kind[None, :]).ravel()                  # the small pair of every big pair
    cnt = runs.ravel()[small].astype(np.int64)
    total = int(cnt.sum())
    pair = np.repeat(np.arange(N * N, dtype=np.int64), cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    out = rec[start[small][pair] + within].copy()
    out["src"], out["dst"] = pair // N, pair % N
    per = np.stack([(v == a).sum(axis=2).ravel() for a in range(4)]).astype(np.uint64)   # [4, n n]
    hist = per[:, small].sum(axis=1).astype(np.uint64)
    return (out, total, runs.ravel()[small].reshape(N, N).astype(np.uint32),
            allow.ravel()[small].reshape(N, N).astype(np.uint32), hist)


# ---- closed forms of the hop search -------------------------------------------

def _dist(name, s, d, n):
    """The hop counts of graph(name, n) for index tensors s, d (int64,
    broadcastable), uncapped; -1 where d is out of reach.  The diagonal is 0."""
    import torch
    s, d = torch.broadcast_tensors(s, d)
    far = torch.full_like(s, -1)
    step = (s != d).long()                               # 0 on the diagonal, 1 off it
    if name == "path":
        return torch.where(d >= s, d - s, far)
    if name == "cycle":
        return (d - s) % n
    if name == "cliques":
        h = (n + 1) // 2
        # first clique -> second: to the bridge's tail h - 1, over it, on from its head h
        over = (s != h - 1).long() + 1 + (d != h).long()
        return torch.where((s < h) == (d < h), step, torch.where(s < h, over, far))
    if name == "star":
        # the centre reaches every leaf; only the odd leaves reach the centre, and the rest through it
        leaf = torch.where(s % 2 == 1, 2 - (d == 0).long(), far)
        return torch.where(s == d, step, torch.where(s == 0, step, leaf))
    if name == "complete":
        return step
    if name == "empty":
        return torch.where(s == d, step, far)
    raise KeyError(name)


def _blocks(n, p=1):
    rows = max(1, BLOCK_CELLS // max(n * p, 1))
    return [(r0, min(n, r0 + rows)) for r0 in range(0, n, rows)]


def _hops_block(name, n, H, r0, r1, device):
    import torch
    s = torch.arange(r0, r1, device=device, dtype=torch.int64)[:, None]
    d = torch.arange(n, device=device, dtype=torch.int64)[None, :]
    x = _dist(name, s, d, n)
    x = torch.where((x < 0) | (x > (H or 254)), torch.full_like(x, NONE), x)
    return x.to(torch.uint8)


def closed_hops(name, n, H=0, device=None):
    """hops_ref(graph(name, n), H) as index arithmetic: [n, n] u8, a numpy
    array (device None: computed on the CPU) or a tensor on `device`;
    evaluated in row blocks."""
    import torch
    dev = torch.device("cpu" if device is None else device)
    out = torch.empty((n, n), dtype=torch.uint8, device=dev)
    for r0, r1 in _blocks(n):
        out[r0:r1] = _hops_block(name, n, H, r0, r1, dev)
    return out.numpy() if device is None else out


def closed_matrix(name, n, p, device=None):
    """A [p, n, n] u8 verdict matrix whose ALLOW cells under some probe, off
    the diagonal, are exactly graph(name, n): every edge is ALLOW under probe
    (s + d) % p and under some of the others, every other cell off the
    diagonal is 0, 1 or 3 under all of them, the diagonal is ALLOW.  numpy
    (device None) or a tensor on `device`; built in row blocks."""
    import torch
    dev = torch.device("cpu" if device is None else device)
    out = torch.empty((p, n, n), dtype=torch.uint8, device=dev)
    for r0, r1 in _blocks(n, p):
        s = torch.arange(r0, r1, device=dev, dtype=torch.int64)[None, :, None]
        d = torch.arange(n, device=dev, dtype=torch.int64)[None, None, :]
        q = torch.arange(p, device=dev, dtype=torch.int64)[:, None, None]
        edge = (_hops_block(name, n, 0, r0, r1, dev) == 1)[None]
        fill = (5 * s + 3 * d + 7 * q) % 3
        fill = fill + (fill == 2).long()                              # 0, 1, 3
        carries = (q == (s + d) % p) | ((3 * s + 5 * d + q) % 4 == 0)
        m = torch.where(edge & carries, torch.full_like(fill, ALLOW), fill)
        m = torch.where(s == d, torch.full_like(m, ALLOW), m)
        out[:, r0:r1] = m.to(torch.uint8)
    return out.numpy() if device is None else out


def closed_sums(hops):
    """reach_hops_cases.sums of a hops tensor, in torch on its device, in row
    blocks: (reach [N] i32, exposed [N] i32, levels [256] i64, closure [N, W]
    i64 -- the u64 words' bits)."""
    import torch
    n = hops.shape[0]
    w = (n + 63) // 64
    dev = hops.device
    reach = torch.empty(n, dtype=torch.int32, device=dev)
    exposed = torch.zeros(n, dtype=torch.int64, device=dev)
    levels = torch.zeros(256, dtype=torch.int64, device=dev)
    closure = torch.empty((n, w), dtype=torch.int64, device=dev)
    # bit k of a word as an int64 (bit 63: the sign bit; the sum of distinct bits never carries)
    weight = torch.tensor([(1 << k) - (1 << 64 if k == 63 else 0) for k in range(64)], dtype=torch.int64, device=dev)
    for r0, r1 in _blocks(n):
        h = hops[r0:r1]
        got = h != NONE
        reach[r0:r1] = (got.sum(dim=1) - 1).to(torch.int32)
        exposed += got.sum(dim=0)
        levels += torch.bincount(h.reshape(-1).to(torch.int32), minlength=256)
        bits = torch.zeros((r1 - r0, w * 64), dtype=torch.int64, device=dev)
        bits[:, :n] = got
        closure[r0:r1] = (bits.reshape(r1 - r0, w, 64) * weight).sum(dim=2)
    return reach, (exposed - 1).to(torch.int32), levels, closure
