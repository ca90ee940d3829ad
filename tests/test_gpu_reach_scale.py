"""The reachability calls on the GPU at the sizes where their kernels and host
code change path (cls_reach_matrix, cls_reach_diff, cls_reach_ports,
cls_reach_hops): waves of reach_reduce inside one row (N >= 256), its
histogram's global-atomic path (a chunk of more than 64 probes), a second turn
of the grid-stride loops, a second tile at the default reach_tile, cell
offsets at and above 2^32, every column-chunk width of reach_hops_bfs up to
W = 512 words per row, the halved block heights, and the port sweep's pair
arithmetic at N >= 256 and over two default tiles.

The references cost index arithmetic (tests/reach_scale_cases.py, each checked
on its own in tests/test_reach_scale_cpu.py): the oracle's 37-endpoint matrix
taken by kinds, the brute-force port ranges taken by kinds, closed-form hop
counts.  Every test asserts the precondition that makes it reach its branch,
with the CU count read from the device.  Whole outputs are compared, bit for
bit; the one exception is stated in test_hops_at_the_maximum."""
import numpy as np
import pytest

import reach_cases as rc
import reach_diff_cases as dc
import reach_hops_cases as hc
import reach_ports_cases as pc
import reach_scale_cases as sc
from test_gpu_reach import _same

pytestmark = pytest.mark.gpu

TILE = 16 << 20                                          # the default reach_tile
CHUNK, LDS_PROBES, HOPS_BLOCK = 4096, 64, 256            # kReachChunk, kReachLdsProbes, kHopsBlock
NAMES = ("hops", "reach", "exposed", "levels", "closure")


@pytest.fixture(scope="module")
def engines():
    """Engines by (family with the case installed, or None for an engine
    without ACLs; options), made on first use and shared by the module's
    tests: (engine, the interface id of every interface of the case)."""
    from vpp_amd.engine import Engine
    made = {}

    def get(fam=None, **opts):
        key = (fam,) + tuple(sorted(opts.items()))
        if key not in made:
            eng = Engine(options=opts or None)
            ids = None
            if fam:
                rc.install(eng, rc.case(fam))
                ids = np.array([eng.if_id(x) for x in rc.case(fam)["ifs"]], np.uint32)
            made[key] = (eng, ids)
        return made[key]
    yield get
    for eng, _ in made.values():
        eng.close()


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _opts(tile):
    return {"reach_tile": tile} if tile else {}


def _matrix(eng, if_ids, b, probes=None, **kw):
    pr, sp, dp = probes or (b["pr"], b["sp"], b["dp"])
    return eng.reach_matrix(if_ids[b["at"]], b["addrs"], pr, sp, dp, **kw)


def _check_matrix(res, want, hist, allow, what):
    v, h, a = res
    if want is not None:
        _same(v, want, what + ": verdicts")
    assert h.dtype == np.uint64 and a.dtype == np.uint32
    _same(h, hist, what + ": hist")
    _same(a, allow, what + ": allow")


def _reset_counters(eng, b):
    for name in b["by_name"]:
        eng.conn_counters(name, reset=True)


def _check_counters(eng, b, counts, what):
    assert sum(int(v.sum()) for v in counts.values()) > 0
    for name in b["by_name"]:
        _same(eng.conn_counters(name, reset=True), counts[name], "%s: counters of %s" % (what, name))


# ---- the matrix ----------------------------------------------------------------

@pytest.mark.parametrize("tile", [None, 1024])
@pytest.mark.parametrize("fam", [4, 16])
def test_matrix_259(fam, tile, engines):
    """m = 7: N = 259 x 3 probes.  N >= 256, so waves of reach_reduce lie in
    one row (allow[row_a] from lane 0 after a wave sum) between waves that
    cross a row end."""
    b = sc.expand(rc.case(fam), 7)
    N, cells = b["N"], 3 * b["N"] ** 2
    assert N == 259 and N >= 256
    per = min(tile or TILE, cells)
    inside = sum(1 for w0 in range(0, per, 256) if w0 % N + 255 < N and w0 + 255 < per)
    assert 0 < inside < per // 256                       # both kinds of wave in a tile
    eng, if_ids = engines(fam, **_opts(tile))
    _check_matrix(_matrix(eng, if_ids, b), b.want(), b["hist"], b["allow"], "N 259, reach_tile %s" % tile)


@pytest.mark.parametrize("fam", [4, 16])
def test_matrix_256(fam, engines):
    """N = 256 exactly, the kinds drawn with repeats (not uniform: the sums
    are those of the matrix by kinds): every wave lies in one row."""
    b = sc.by_kinds(rc.case(fam), sc.drawn(256))
    assert b["N"] == 256 and TILE % 256 == 0
    hist, allow = sc.sums(b.want())
    assert rc.diverse(b.want())
    eng, if_ids = engines(fam)
    _check_matrix(_matrix(eng, if_ids, b), b.want(), hist, allow, "N 256")


@pytest.mark.parametrize("tile", [None, 1024])
@pytest.mark.parametrize("fam", [4, 16])
def test_matrix_200_probes(fam, tile, engines):
    """N = 5, P = 200 (the case's probes cyclically): a chunk of 4,096 cells
    spans more than 64 probes, so reach_reduce's histogram leaves its LDS bins
    for global atomics, in the per-lane path (no wave lies in one probe)."""
    b = sc.by_kinds(rc.case(fam), np.arange(5))
    P, N = 200, 5
    probes = sc.cyclic(b, P)
    want = np.ascontiguousarray(b.want()[np.arange(P) % 3])
    assert 256 > N * N and P * N * N > CHUNK
    if tile is None:
        assert CHUNK // (N * N) > LDS_PROBES + 2 and P > LDS_PROBES + 2      # a chunk spans more than 64 probes
    else:
        assert tile % (N * N) and P * N * N > 4 * tile                      # tiles that begin inside a later probe
    assert len(np.unique(want)) >= 3
    hist, allow = sc.sums(want)
    eng, if_ids = engines(fam, **_opts(tile))
    _check_matrix(_matrix(eng, if_ids, b, probes), want, hist, allow, "5 x 200, reach_tile %s" % tile)
    v, h, a = _matrix(eng, if_ids, b, probes, verdicts=False)
    assert v is None
    _check_matrix((None, h, a), None, hist, allow, "5 x 200, reach_tile %s, no verdicts" % tile)


@pytest.mark.parametrize("fam", [4, 16])
def test_matrix_two_default_tiles(fam, engines):
    """m = 64: N = 2,368 x 3 probes = 16,822,272 cells -- two tiles at the
    default reach_tile, the last of 45,056 cells, and more chunks than
    reach_reduce has workgroups, so its grid-stride loop (and those of
    reach_expand4/16) takes a second turn.  One counting call: verdicts, hist,
    allow and the connection counters."""
    b = sc.expand(rc.case(fam), 64)
    cells = 3 * b["N"] ** 2
    assert cells == 16822272 and cells > TILE and cells - TILE == 45056
    assert cells > 8 * _n_cu() * CHUNK and TILE > 8 * _n_cu() * CHUNK
    eng, if_ids = engines(fam)
    _reset_counters(eng, b)
    res = _matrix(eng, if_ids, b, count=True)
    _check_matrix(res, b.want(), b["hist"], b["allow"], "N 2368")
    _check_counters(eng, b, b["counts"], "N 2368")


@pytest.mark.parametrize("fam", [4, 16])
def test_matrix_above_2_32_cells(fam, engines):
    """m = 1024: N = 37,888 x 3 probes = 4,306,501,632 cells, the smallest
    uniform case above 2^32: the last tiles' cell offsets `first` need 64 bits
    (row = first / N, T.p0, r_allow + row, r_hist + 4 p0).  No verdicts; hist
    (m^2 x) and all P N allow counts (m x); IPv4 also counts."""
    b = sc.expand(rc.case(fam), 1024)
    cells = 3 * b["N"] ** 2
    assert cells == 4306501632 and cells > 1 << 32 and (cells - 1) // TILE * TILE >= 1 << 32
    eng, if_ids = engines(fam)
    v, h, a = _matrix(eng, if_ids, b, verdicts=False)
    assert v is None and a.shape == (3, b["N"]) and int(h.sum()) == cells
    _check_matrix((None, h, a), None, b["hist"], b["allow"], "N 37888")
    if fam == 4:
        _reset_counters(eng, b)
        v, h, a = _matrix(eng, if_ids, b, verdicts=False, count=True)
        _check_matrix((None, h, a), None, b["hist"], b["allow"], "N 37888, counting")
        _check_counters(eng, b, b["counts"], "N 37888")


# ---- the diff ------------------------------------------------------------------

@pytest.mark.parametrize("m", [7, 64])
@pytest.mark.parametrize("fam", [4, 16])
def test_diff(fam, m, engines):
    """The host form against a baseline that differs in a seeded 1 % of the
    cells and at the chunk and tile ends: the total, every record (cap above
    the total), trans and changed equal diff_ref.  At m = 64 the records
    straddle the default tile boundary."""
    b = sc.expand(rc.case(fam), m)
    want = b.want()
    cells = want.size
    base = np.array(want)
    rng = np.random.default_rng(83 + m)
    base[rng.random(want.shape) < 0.01] ^= 2
    ends = sorted({0, CHUNK - 1, CHUNK, min(TILE, cells) - 1, min(TILE, cells - 1), cells - 1})
    base.reshape(-1)[ends] ^= 0x41
    rec, total, trans, changed = dc.diff_ref(base, want)
    assert cells // 128 < total < cells // 64
    flat = (rec["probe"].astype(np.int64) * b["N"] + rec["src"]) * b["N"] + rec["dst"]
    assert set(ends) <= set(flat.tolist())
    if m == 64:
        assert cells > TILE and (flat < TILE).sum() > 1000 and (flat >= TILE).sum() > 100
        assert cells > 8 * _n_cu() * CHUNK
    eng, if_ids = engines(fam)
    r = eng.reach_diff(if_ids[b["at"]], b["addrs"], b["pr"], b["sp"], b["dp"], base, cap=total + 8)
    assert r.n_changes == total and len(r.changes) == total
    for f in ("probe", "src", "dst", "was", "now"):
        _same(r.changes[f], rec[f], "m %d: records' %s" % (m, f))
    assert r.changes.tobytes() == rec.tobytes()
    _same(r.verdicts, want, "m %d: verdicts" % m)
    _same(r.trans, trans, "m %d: trans" % m)
    _same(r.changed, changed, "m %d: changed" % m)


# ---- the port sweep --------------------------------------------------------------

def _ports(fam, m, tile, engines):
    c = rc.case(fam)
    eps, v = pc.brute(fam, 0)
    kind = sc.kinds(m, 2, pc.N_BRUTE)
    at = eps[kind]                                       # the case's endpoint of every swept one
    eng, if_ids = engines(fam, **_opts(tile))
    r = eng.reach_ports(if_ids[c["at"][at]], c["addrs"][at], 0, pc.SPORT[0])
    rec, total, runs, allow, hist = sc.ports_by_kinds(v, kind)
    N = len(kind)
    assert r.n_classes == len(pc.class_starts(pc.bound_rules(c, eps), 0))
    assert r.n_ranges == total and len(r.ranges) == total
    for f in ("src", "dst", "port_lo", "port_hi", "action", "zero"):
        _same(r.ranges[f], rec[f], "ranges' %s" % f)
    _same(r.runs, runs, "runs")
    _same(r.allow_ports, allow, "allow_ports")
    _same(r.hist, hist, "hist")
    assert int(r.hist.sum()) == 65536 * N * N and runs.max() > 1
    return r.n_classes, N


@pytest.mark.parametrize("m", [43, 67])
@pytest.mark.parametrize("fam", [4, 16])
def test_ports(fam, m, engines):
    """The brute force's six endpoints as kinds, protocol 0.  m = 43: N = 258
    >= 256 in ports_row's two divisions.  m = 67: N = 402, where K N^2 is
    more than one default tile for both families (K = 105 and 195 classes:
    at N = 258 it is not), so the pair-major tiling of whole pairs has a second
    tile."""
    K, N = _ports(fam, m, None, engines)
    assert N >= 256
    if m == 67:
        assert K * N * N > TILE and TILE // K < N * N
        assert TILE // K * K > 8 * _n_cu() * CHUNK                          # a second turn of the sweep's loops


def test_ports_tiles_of_1024_rows(engines):
    """N = 258 with reach_tile 1024: a few whole pairs per tile."""
    K, N = _ports(4, 43, 1024, engines)
    assert N >= 256 and 1 <= 1024 // K < 16


# ---- the hop closure, evaluating form -----------------------------------------------

def _check_hops(r, hops, what):
    want = (hops,) + hc.sums(hops)
    for name, g, w in zip(NAMES, r, want):
        assert g.dtype == w.dtype, (what, name, g.dtype)
        _same(g, w, "%s: %s" % (what, name))
    n = len(hops)
    if n % 64:
        assert not (r.closure[:, -1] >> np.uint64(n % 64)).any(), what + ": closure padding"


@pytest.mark.parametrize("tile", [None, 1024])
@pytest.mark.parametrize("m", [7, 28])
@pytest.mark.parametrize("fam", [4, 16])
def test_hops_evaluating_form(fam, m, tile, engines):
    """m = 7 (N = 259, W = 5) and m = 28 (N = 1,036, W = 17: a second pass
    over a word's frontier bits): the matrix is evaluated and folded tile by
    tile; every output equals hops_ref of the matrix by kinds and its sums."""
    b = sc.expand(rc.case(fam), m)
    N = b["N"]
    assert (N + 63) // 64 == {7: 5, 28: 17}[m]
    hops = hc.hops_ref(hc.adjacency(b.want()))
    lv = hc.sums(hops)[2]
    assert int(np.flatnonzero(lv[:255]).max()) <= 4 and lv[1] and lv[2] and lv[255]    # a few levels: cheap products
    if m == 28 and tile is None:
        assert 3 * N * N > 8 * _n_cu() * 256             # reach_adj_fold's grid-stride loop takes a second turn
    eng, if_ids = engines(fam, **_opts(tile))
    r = eng.reach_hops(if_ids[b["at"]], b["addrs"], b["pr"], b["sp"], b["dp"], closure=True)
    _check_hops(r, hops, "m %d, reach_tile %s" % (m, tile))


# ---- the hop closure, matrix form -------------------------------------------------

def _cw(W):
    """The search's column chunk CW and its frontier-bit groups G."""
    cw = 1
    while cw < W and cw < HOPS_BLOCK:
        cw *= 2
    return cw, HOPS_BLOCK // cw


def _fold_device(eng, m, hops=True):
    import torch
    r = eng.reach_hops(None, None, None, None, None, matrix=m, hops=hops, closure=True, out=(None,) * 5)
    torch.cuda.synchronize()
    return r


def _check_device(r, want_hops, what, hops=True):
    """A device-form result against a device hops reference and its sums,
    compared on the device."""
    import torch
    n = want_hops.shape[0]
    reach, exposed, levels, closure = sc.closed_sums(want_hops)
    if hops:
        assert r.hops.dtype == torch.uint8 and r.hops.shape == (n, n)
        bad = int((r.hops != want_hops).sum())
        assert bad == 0, (what, "hops", bad, (r.hops != want_hops).nonzero()[:8].tolist())
    for name, g, w in (("reach", r.reach, reach), ("exposed", r.exposed, exposed), ("levels", r.levels, levels),
                       ("closure", r.closure, closure)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, g.dtype)
        bad = int((g != w).sum())
        assert bad == 0, (what, name, bad, (g != w).nonzero()[:8].tolist())
    if n % 64:
        assert not bool(((r.closure[:, -1] >> (n % 64)) != 0).any()), what + ": closure padding"
    assert int(levels[0]) == n and int(levels.sum()) == n * n


@pytest.mark.parametrize("n, W", [(513, 9), (1025, 17), (4097, 65), (8193, 129), (16384, 256), (16385, 257)])
def test_hops_closed_forms(n, W, engines):
    """Every closed-form graph in the matrix form: W = 9 (G = 16, all four
    bits of a group live), 17 (a second pass over a word's bits), 65, 129
    (G = 1: every thread in group 0), 256 and 257 (a second column chunk with
    idle lanes, and the per-word loops taking a second turn).  Host matrices
    of three probes up to N = 1,025, then device matrices of one."""
    import torch
    assert (n + 63) // 64 == W
    cw, G = _cw(W)
    assert (cw, G) == {9: (16, 16), 17: (32, 8), 65: (128, 2), 129: (256, 1), 256: (256, 1), 257: (256, 1)}[W]
    assert (W > cw) == (W == 257) and (W > HOPS_BLOCK) == (W == 257)
    eng, _ = engines()
    for name in sc.CLOSED:
        what = "%s %d" % (name, n)
        if n <= 1025:
            m = sc.closed_matrix(name, n, 3)
            hops = sc.closed_hops(name, n)
            r = eng.reach_hops(None, None, None, None, None, matrix=m, closure=True)
            _check_hops(r, hops, what)
        else:
            m = sc.closed_matrix(name, n, 1, device="cuda")
            _check_device(_fold_device(eng, m), sc.closed_hops(name, n, device="cuda"), what)
            del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["cliques", "star"])
def test_hops_at_the_maximum(name, engines):
    """N = 32,768, the call's maximum (W = 512): reach, exposed, levels and
    the closure against the closed form.  The hops array (1 GiB) is not asked
    for: the one output this module leaves out."""
    import torch
    n = 32768
    eng, _ = engines()
    m = sc.closed_matrix(name, n, 1, device="cuda")
    r = _fold_device(eng, m, hops=False)
    assert r.hops is None
    _check_device(r, sc.closed_hops(name, n, device="cuda"), "%s %d" % (name, n), hops=False)
    del m, r
    torch.cuda.empty_cache()


def _hops_lds(n, rows):
    W = (n + 63) // 64
    return (3 * rows * W + W) * 8 + 256 * 4


@pytest.mark.parametrize("n, rows", [(16385, 16), (20673, 8), (20673, 16)])
def test_hops_rows_halved(n, rows, engines):
    """hops_rows 16 at W = 257 and 8 and 16 at W = 324: the rows asked for do
    not fit 64 KiB of LDS and are halved (16 -> 8 from W = 165, 8 -> 4 from
    W = 323).  The outputs equal the closed form and the default engine's."""
    import torch
    W = (n + 63) // 64
    assert W == {16385: 257, 20673: 324}[n]
    assert _hops_lds(n, rows) > 65536 and _hops_lds(n, 4) <= 65536
    if rows == 16:
        assert (_hops_lds(n, 8) <= 65536) == (n == 16385)
    eng, _ = engines(None, hops_rows=rows)
    plain, _ = engines()
    for name in ("cliques", "star", "cycle"):
        what = "%s %d, hops_rows %d" % (name, n, rows)
        m = sc.closed_matrix(name, n, 1, device="cuda")
        r = _fold_device(eng, m)
        _check_device(r, sc.closed_hops(name, n, device="cuda"), what)
        d = _fold_device(plain, m)
        for k, (x, y) in enumerate(zip(r, d)):
            assert torch.equal(x, y), (what, NAMES[k], "against the default engine")
        del m, r, d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", [513, 1025])
def test_hops_sparse_frontiers(n, engines):
    """random1 / random2 (out-degree about 2) against hops_ref: frontiers of a
    few bits per word, where most groups of four bits are skipped."""
    eng, _ = engines()
    for name in ("random1", "random2"):
        m, a = hc.synthetic(name, n, 3)
        hops = hc.synthetic_ref(name, n)[0]
        lv = hc.sums(hops)[2]
        assert a.sum() < 3 * n and np.flatnonzero(lv[:255]).max() >= 6       # sparse, and many levels
        r = eng.reach_hops(None, None, None, None, None, matrix=np.ascontiguousarray(m), closure=True)
        _check_hops(r, hops, "%s %d" % (name, n))
