"""The rule necessity sweep on the GPU at the sizes where its waves loop
(cls_table_need; need_cells, need_bits, need_mark, need_free and need_finish of
k_need.hip, and cover_fold of k_cover.hip above two steps per wave).

The shapes are tests/need_scale_cases.py's, and tests/test_need_scale_cpu.py
asserts on the reference what each is for: first matches in every stride of
4,096 rules, second matches in the same stride and one to three strides on,
at least 100 DEAD, REDUNDANT and NEEDED rules and ten REDUNDANT ones that are
not free, T above 64 and no multiple of it, the column rows' size against the
80 KiB and 144 KiB of launch_cells.  Here every case asserts, with the CU
count read from the device, that the pairs outnumber the waves launch_cells
starts, and then bit-exact equality of every output (need, free, first,
changed, witness, counts, n_cells, dims) with Engine.table_need_host.

    shape  R       W    form  Ks x Kd = pairs     T    cells      column rows
    a      1,000   16   NW 1  283 x 258 = 73,014  28   2,044,392  3.5 KiB
    b      4,096   64   NW 1  154 x 134 = 20,636  84   1,733,424  42.0 KiB
    c      4,097   65   NW 2  154 x 134 = 20,636  84   1,733,424  42.7 KiB
    c_odd  4,097   65   NW 2  154 x 134 = 20,636  85   1,754,060  43.2 KiB
    d      8,100   127  NW 2  124 x 104 = 12,896  140  1,805,440  138.9 KiB
    e      12,000  188  NW 4  124 x 104 = 12,896  68   876,928    99.9 KiB
    f      16,000  250  NW 4  124 x 104 = 12,896  68   876,928    132.8 KiB
    g      16,450  258  NW 0  144 x 114 = 16,416  68   1,116,288  137.1 KiB
    h      16,450  258  NW 0  124 x 104 = 12,896  148  1,908,608  298.3 KiB (global memory)
    fold   1,000   16   NW 1  283 x 258 = 73,014  76   5,549,064  9.5 KiB

Measured on an MI355X: the module's 27 tests take 8.6 s in all; the slowest
is test_shape[f] at 0.78 s (the first test also installs nothing shared but
pays 1.7 s of engine setup), test_fold_three_steps 0.44 s."""
import numpy as np
import pytest

import cover_cases as cc
import need_cases as nc
import need_scale_cases as ns
from vpp_amd.engine import Engine, minimize_rounds

pytestmark = pytest.mark.gpu

TILE = 16 << 20                                          # the default cover_tile
NAMES = ("need", "free", "first", "changed", "witness", "counts")


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def tables(eng):
    """The shapes' tables, installed on first use and shared by the module's tests."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = eng.put_table("scale " + name, ns.shape(name))
        return made[name]
    yield get
    for t in made.values():
        eng.del_table(t)


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _geometry(name):
    return ns.geometry(ns.host(name), len(ns.shape(name)))


def _sweep(eng, tb, want, what, skip=None, tile=None, lds=None):
    eng.set_option("cover_tile", tile)
    eng.set_option("need_cols_lds", lds)
    try:
        got = eng.table_need(tb, skip=skip)
    finally:
        eng.set_option("cover_tile", None)
        eng.set_option("need_cols_lds", None)
    nc.same_results(got, want, what)
    assert int(got["first"].sum()) == got["n_cells"], what
    return got


# ---- every shape at the default tile ------------------------------------------------

@pytest.mark.parametrize("name", ns.MAIN + ("c_odd",))
def test_shape(eng, tables, name):
    """One tile; the pair loop `pair += gridDim.x * kCellsWaves` takes at
    least 2.5 passes, the last one ragged.  Shape h's rows are above
    kColsLdsMax: global memory without the option, two workgroups per CU, so
    a second, ragged pass only."""
    t, w, pairs, cells, col_bytes = _geometry(name)
    assert ns.tiles(pairs, t, TILE)[1] == 1
    waves = ns.cells_waves(pairs, _n_cu(), col_bytes)
    per_cu = waves // (ns.CELLS_WAVES * _n_cu())
    assert per_cu == (1 if name in ("d", "e", "f", "g") else 2)
    if name == "h":
        assert col_bytes > ns.LDS_MAX and pairs > waves and pairs % waves
    else:
        assert pairs >= 2.5 * waves and pairs % waves
    _sweep(eng, tables(name), ns.host(name), name)


@pytest.mark.parametrize("name", ["c", "e", "g"])
def test_columns_from_global_memory(eng, tables, name):
    """need_cols_lds 0 on NW 2, NW 4 and NW 0: two workgroups per CU whatever
    the rows' size, a second pass of the pair loop on each."""
    t, w, pairs, cells, col_bytes = _geometry(name)
    waves = ns.cells_waves(pairs, _n_cu(), col_bytes, lds=False)
    assert waves == 2 * ns.CELLS_WAVES * _n_cu() and pairs > waves and pairs % waves
    if name == "c":
        assert pairs >= 2.5 * waves
    _sweep(eng, tables(name), ns.host(name), name + " lds 0", lds=0)


# ---- tiles with pair0 != 0 --------------------------------------------------------------

@pytest.mark.parametrize("name, tile", [("b", 1 << 20), ("b", 1 << 18), ("g", 1 << 20), ("g", 1 << 19), ("g", 1 << 18)])
def test_tiles(eng, tables, name, tile):
    """Later tiles begin at pair0 != 0 and the last tile is ragged.  Shape g at
    2^19 cells: a full later tile in which the pair loop takes a second pass."""
    t, w, pairs, cells, col_bytes = _geometry(name)
    per, n, last = ns.tiles(pairs, t, tile)
    assert n >= 2 and 0 < last < per
    if (name, tile) == ("g", 1 << 19):
        assert n >= 3 and per > ns.cells_waves(per, _n_cu(), col_bytes)
    _sweep(eng, tables(name), ns.host(name), "%s tile %d" % (name, tile), tile=tile)


# ---- skip ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["b", "g"])
def test_skip(eng, tables, name):
    """A random third of the rules deleted (bits cleared and kept in every
    word of the kept row), then the free rules (the second round)."""
    third = ns.skip_third(name)
    _sweep(eng, tables(name), ns.host(name, third, "third"), name + " skip a third", skip=third)
    free = np.flatnonzero(ns.host(name)["free"]).tolist()
    assert len(free) >= 100
    _sweep(eng, tables(name), ns.host(name, free, "free"), name + " skip the free rules", skip=free)


# ---- the device form ----------------------------------------------------------------------

def test_device_form(eng, tables):
    """Shape g into torch outputs on a side stream."""
    import torch
    want = ns.host("g")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = eng.table_need(tables("g"), out=(None,) * 6, stream=side)
    assert got["n_cells"] == want["n_cells"] and got["dims"] == want["dims"]
    side.synchronize()
    for name in NAMES:
        assert got[name].cpu().numpy().tobytes() == want[name].tobytes(), name


# ---- ties to the coverage sweep, the table diff and the round loop ------------------------

@pytest.mark.parametrize("name", ["b", "g"])
def test_tie_to_cover(eng, tables, name):
    want = ns.host(name)
    r = len(ns.shape(name))
    cov = eng.table_cover(tables(name), af=4)
    assert cov["n_cells"] == want["n_cells"] and cov["dims"] == want["dims"]
    assert np.array_equal(cov["cells"], want["first"])
    assert np.array_equal(cov["live"][:r] == 0, want["need"] == ns.DEAD)
    assert cov["n_dead"] == want["counts"][ns.DEAD]


@pytest.mark.parametrize("name", ["b", "g"])
def test_tie_to_diff(eng, tables, name):
    """The list without r against the list, for six rules: NEEDED ones whose
    fall-through rule lies in another stride (shape g) or is any rule, a
    REDUNDANT and a DEAD one; then the list without all free rules."""
    rules = ns.shape(name)
    n = len(rules)
    ta = tables(name)
    got = _sweep(eng, ta, ns.host(name), name)
    need, wit = got["need"], got["witness"]
    k = np.arange(n)
    rng = np.random.default_rng(n)
    falls = (need == ns.NEEDED) & (wit["fall"] < n)
    far = falls & (wit["fall"] >> 12 != k >> 12) if n > ns.STRIDE else falls & (wit["fall"] - k > 64)
    some = [int(x) for m, c in ((far, 2), (falls, 1), (need == ns.NEEDED, 1), (need == ns.REDUNDANT, 1), (need == ns.DEAD, 1))
            for x in rng.choice(np.flatnonzero(m), c, replace=False)]
    assert len(set(some)) == 6
    for r in some:
        tb = eng.put_table("tie without", rules[:r] + rules[r + 1:])
        try:
            d = eng.table_diff(ta, tb, rec_cap=1)
        finally:
            eng.del_table(tb)
        assert d["equal"] == (need[r] != ns.NEEDED), r
        if not d["equal"]:
            rec, w = d["records"][0], wit[r]
            assert (rec["src_lo"], rec["dst_lo"], rec["proto"], rec["port_lo"]) == \
                (w["src"], w["dst"], w["proto"], w["dport"]), r
            assert rec["rule_a"] == r and rec["now"] == w["after"] & 3 and w["after"] & 0x80
            assert rec["rule_b"] + (1 if rec["rule_b"] >= r else 0) == w["fall"], r
            f = d["first"]
            assert (f["src"], f["dst"], f["proto"], f["dport"]) == (w["src"], w["dst"], w["proto"], w["dport"])
    keep = np.flatnonzero(got["free"] == 0)
    assert len(keep) < n - 100
    tb = eng.put_table("tie free", [rules[i] for i in keep])
    try:
        assert eng.table_diff(ta, tb, rec_cap=0)["equal"]
    finally:
        eng.del_table(tb)


@pytest.mark.parametrize("name", ["b", "g"])
def test_tie_round_loop(eng, tables, name):
    """minimize_rounds over the device sweep and over the host form: the same
    kept rules and the same rounds, more than one of them."""
    rules = ns.shape(name)
    cr = nc._abi.CRules(rules)
    dev = minimize_rounds(lambda skip: eng.table_need(tables(name), skip=skip), len(rules))
    hst = minimize_rounds(lambda skip: Engine.table_need_host(cr, skip=skip), len(rules))
    assert dev == hst
    assert len(dev[1]) >= 2 and len(dev[0]) >= 100


# ---- cover_fold above two steps per wave -------------------------------------------------

def test_fold_three_steps(eng, tables):
    """Shape a's networks with 18 port ranges (T = 76): one tile of 5.5 M
    cells, n / (2 n_cu 16 256) >= 2.5 steps per wave of cover_fold (the cover,
    diff and need tests stop at 2^22 cells: two).  table_need against the host
    form; table_cover's cells, live and n_dead against the host form's first,
    its witnesses against the first cell per rule of Engine.classify_rules over
    every cell (numpy), that pinned to the oracle on 4,096 sampled cells."""
    rules = ns.shape("fold")
    r = len(rules)
    want = ns.host("fold")
    n = want["n_cells"]
    assert 2.5 * ns.FOLD_STEP_CELLS * _n_cu() <= n <= TILE
    tb = tables("fold")
    _sweep(eng, tb, want, "fold")
    cov = eng.table_cover(tb, af=4)
    assert cov["n_cells"] == n and cov["dims"] == want["dims"]
    assert np.array_equal(cov["cells"], want["first"])
    assert np.array_equal(cov["live"], (want["first"] > 0).astype(np.uint8))
    assert cov["n_dead"] == want["counts"][ns.DEAD]
    c = ns.cells(rules)
    assert len(c["src"]) == n
    hit = eng.classify_rules(tb, c["src"], c["dst"], c["dport"], c["proto"])[1].astype(np.int64)
    at = np.random.default_rng(76).choice(n, 4096, replace=False)
    assert np.array_equal(cc.oracle_rules(rules, {f: np.ascontiguousarray(c[f][at]) for f in nc.FIELDS}), hit[at])
    assert np.array_equal(np.bincount(hit, minlength=r + 1), want["first"])
    wit = np.zeros(r + 1, nc._abi.COVER_WITNESS)
    k, first = np.unique(hit, return_index=True)          # the first (lowest) cell of each rule hit
    for f in nc.FIELDS:
        wit[f][k] = c[f][first]
    wit["live"][k] = 1
    assert len(k) == int((want["first"] > 0).sum()) >= 800 and first.max() > n // 2
    assert cov["witness"].tobytes() == wit.tobytes()
