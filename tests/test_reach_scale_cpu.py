"""The scale tests' references on their own (tests/reach_scale_cases.py), at
sizes where the oracle and hops_ref are affordable: the matrix by kinds against
the C oracle over the really expanded rows, the closed-form hop counts,
matrices and sums against reach_hops_cases, the port ranges by kinds against
ranges_ref of the really expanded array.  No GPU."""
import numpy as np
import pytest

import reach_cases as rc
import reach_hops_cases as hc
import reach_ports_cases as pc
import reach_scale_cases as sc

SIZES = (1, 2, 3, 63, 64, 65, 129, 300)


@pytest.mark.parametrize("fam", [4, 16])
def test_matrix_by_kinds_equals_the_oracle(fam):
    """m = 2 (74 endpoints, 16,428 cells): want_big is the oracle's matrix
    over the expanded rows; the multiplied hist, allow and counts are that
    matrix's sums and the oracle's counters."""
    from test_gpu_connect_scale import oracle_connections
    c = rc.case(fam)
    b = sc.expand(c, 2)
    assert b["N"] == 74 and sorted(np.bincount(b["kind"]).tolist()) == [2] * 37
    assert (b["kind"] != np.repeat(np.arange(37), 2)).any()             # shuffled
    si, di, tr = sc.rows_of(b)
    want, counts = oracle_connections(b["bind"], b["by_name"], b["ifs"], si, di, tr, fam)
    want = want.reshape(3, 74, 74)
    assert np.array_equal(b.want(), want)
    assert not b.want().flags.writeable and b.want() is b.want()
    hist, allow = sc.sums(want)
    assert b["hist"].dtype == np.uint64 and np.array_equal(b["hist"], hist)
    assert b["allow"].dtype == np.uint32 and np.array_equal(b["allow"], allow)
    assert counts.keys() == b["counts"].keys()
    for name in counts:
        assert np.array_equal(b["counts"][name], counts[name]), name
    assert sc.expand(c, 2) is b


def test_drawn_kinds_and_cyclic_probes():
    """drawn(): every kind occurs, not uniformly; cyclic(): the case's probes
    in turn."""
    k = sc.drawn(256)
    n = np.bincount(k, minlength=37)
    assert len(k) == 256 and n.min() >= 1 and n.max() > n.min()
    b = sc.by_kinds(rc.case(4), sc.drawn(5))
    pr, sp, dp = sc.cyclic(b, 200)
    assert pr[:4].tolist() == [0, 1, 47, 0] and len(pr) == len(sp) == len(dp) == 200
    assert b.want().shape == (3, 5, 5)


@pytest.mark.parametrize("n", SIZES)
def test_closed_hops_equal_the_search(n):
    """closed_hops and closed_sums against hops_ref and sums of graph(name, n),
    every closed-form graph and H in {0, 1, 3, 254}."""
    import torch
    for name in sc.CLOSED:
        for H in (0, 1, 3, 254):
            want = hc.synthetic_ref(name, n, H)
            got = sc.closed_hops(name, n, H)
            assert got.dtype == np.uint8 and np.array_equal(got, want[0]), (name, n, H)
            if H in (0, 3):
                r, e, lv, cl = sc.closed_sums(torch.from_numpy(got))
                assert np.array_equal(r.numpy().view(np.uint32), want[1]), (name, n, H)
                assert np.array_equal(e.numpy().view(np.uint32), want[2]), (name, n, H)
                assert np.array_equal(lv.numpy().view(np.uint64), want[3]), (name, n, H)
                assert np.array_equal(cl.numpy().view(np.uint64), want[4]), (name, n, H)


def test_closed_hops_in_row_blocks(monkeypatch):
    """Blocks of a few rows give the same arrays as one block."""
    import torch
    whole = {name: (sc.closed_hops(name, 129), sc.closed_matrix(name, 129, 3)) for name in sc.CLOSED}
    monkeypatch.setattr(sc, "BLOCK_CELLS", 129 * 3 * 7)
    assert len(sc._blocks(129, 3)) > 10 and len(sc._blocks(129)) > 4
    for name, (h, m) in whole.items():
        assert np.array_equal(sc.closed_hops(name, 129), h), name
        assert np.array_equal(sc.closed_matrix(name, 129, 3), m), name
        one = hc.sums(h)
        got = sc.closed_sums(torch.from_numpy(h))
        for g, w in zip(got, one):
            assert np.array_equal(g.numpy().view(w.dtype), w), name


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_closed_matrix_holds_the_graph(n, p):
    """closed_matrix's adjacency is graph(name, n); its diagonal is ALLOW, its
    other cells are 0, 1 and 3; with three probes no probe holds every edge."""
    for name in sc.CLOSED:
        m = sc.closed_matrix(name, n, p)
        assert m.shape == (p, n, n) and m.dtype == np.uint8
        a = hc.graph(name, n)
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(hc.adjacency(m) & off, a), (name, n, p)
        assert (m[:, ~off] == sc.ALLOW).all()
        rest = m[:, off & ~a]
        assert np.isin(rest, (0, 1, 3)).all()
        if n >= 63 and name != "complete":
            assert len(np.unique(rest)) == 3, (name, n, p)
        if p == 3 and a.sum() > 8:
            assert all(((m[q] == sc.ALLOW) & a).sum() < a.sum() for q in range(p)), (name, n)


@pytest.mark.parametrize("fam", [4, 16])
def test_port_ranges_by_kinds(fam):
    """6 kinds x 2: the by-kinds records, runs, ALLOW ports and histogram equal
    ranges_ref of the really expanded [12, 12, 65536] array."""
    _, v = pc.brute(fam, 0)
    kind = sc.kinds(2, 1, pc.N_BRUTE)
    assert len(kind) == 12 and (kind != np.repeat(np.arange(6), 2)).any()
    want = pc.ranges_ref(v[kind][:, kind])
    got = sc.ports_by_kinds(v, kind)
    assert got[1] == want[1] and got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes()
    for g, w in zip(got[2:], want[2:]):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert want[2].max() > 1
