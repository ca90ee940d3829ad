"""The rule necessity sweep's scale shapes without a GPU
(tests/need_scale_cases.py): the generator's dimensions, the conditions that
make each shape reach what it is for -- asserted on the reference
(Engine.table_need_host), so that a vacuous GPU case fails here first -- and
the reference itself against literal_for_rule, the check written from the
Python rule fields alone, on 64 sampled narrow rules per shape."""
import numpy as np
import pytest

import cover_cases as cc
import need_scale_cases as ns

# (Ks, Kd, Kt, Ku) of every shape
DIMS = {"a": (283, 258, 13, 13), "b": (154, 134, 41, 41), "c": (154, 134, 41, 41), "c_odd": (154, 134, 42, 41),
        "d": (124, 104, 69, 69), "e": (124, 104, 33, 33), "f": (124, 104, 33, 33), "g": (144, 114, 33, 33),
        "h": (124, 104, 73, 73), "fold": (283, 258, 37, 37)}
WORDS = {"a": 16, "b": 64, "c": 65, "c_odd": 65, "d": 127, "e": 188, "f": 250, "g": 258, "h": 258, "fold": 16}
ALL = ns.MAIN + ("c_odd",)


@pytest.mark.parametrize("name", sorted(ns.SHAPES))
def test_dimensions(name):
    rules = ns.shape(name)
    want = ns.host(name)
    r = len(rules)
    assert r == ns.SHAPES[name][0] and len(want["need"]) == r
    assert cc.dims(rules)[0] == DIMS[name] == want["dims"]           # the Python restatement and the library agree
    t, w, pairs, cells, col_bytes = ns.geometry(want, r)
    assert w == WORDS[name] and cells == want["n_cells"] == int(want["first"].sum())
    assert t == 4 * ns.SHAPES[name][3] + 4 + (1 if ns.SHAPES[name][5] else 0)
    # the register form of need_cells: NW 1, 2, 4, and 0 above 256 words
    strides = (w + 63) // 64
    assert strides == {"a": 1, "b": 1, "c": 2, "c_odd": 2, "d": 2, "e": 3, "f": 4, "g": 5, "h": 5, "fold": 1}[name]
    # the column rows: in LDS two workgroups per CU, one above 80 KiB, none above 144 KiB
    if name in ("a", "b", "c", "c_odd", "fold"):
        assert col_bytes <= ns.LDS_TWO_PER_CU
    elif name == "h":
        assert col_bytes > ns.LDS_MAX
    else:
        assert ns.LDS_TWO_PER_CU < col_bytes <= ns.LDS_MAX
    if name in ("b", "c", "c_odd", "d", "e"):
        assert t > 64 and t % 64                                     # two rounds of 64 columns, the last one partial
    if name == "c_odd":
        assert t % 2 == 1 and w % 2 == 1                             # the odd last word of the LDS copy
    if name == "b":
        assert r % 64 == 0                                           # the last word full
    # the pair loop: passes at 256 CUs (the GPU tests assert them on the device's count)
    assert pairs >= {"a": 70000, "b": 20000, "c": 20000, "c_odd": 20000, "fold": 70000}.get(name, 12000)
    if name == "fold":
        assert cells >= 2.5 * ns.FOLD_STEP_CELLS * 256               # three cover_fold steps per wave at 256 CUs


@pytest.mark.parametrize("name", ALL)
def test_conditions(name):
    """What a shape must have to test anything new, on the reference."""
    rules = ns.shape(name)
    want = ns.host(name)
    r = len(rules)
    need, free, first, wit = want["need"], want["free"], want["first"], want["witness"]
    k = np.arange(r)
    strides = (r + ns.STRIDE - 1) // ns.STRIDE
    assert want["counts"][ns.SKIPPED] == 0 and all(want["counts"][v] >= 100 for v in (ns.DEAD, ns.REDUNDANT, ns.NEEDED))
    assert int(((need == ns.REDUNDANT) & (free == 0)).sum()) >= 10
    assert first[r] > 0                                              # the default has cells
    live = np.bincount(k[first[:r] > 0] >> 12, minlength=strides)
    assert np.all(live > 0), live                                    # a first match in every stride
    needed = need == ns.NEEDED
    fall = wit["fall"].astype(np.int64)
    if strides > 1:
        assert int((needed & (fall >> 12 != k >> 12)).sum()) >= 100
        assert int((needed & (fall >> 12 == k >> 12)).sum()) >= 100
    if name in ("c", "c_odd"):
        # the one rule of the second register: a first match, and what at least ten needed rules fall to
        assert first[4096] > 0 and int((needed & (fall == 4096)).sum()) >= 10
    if strides > 2:
        # a second match that is a rule of another stride, and of a stride two or three on
        rule = needed & (fall < r)
        assert int((rule & (fall >> 12 != k >> 12)).sum()) >= 100
        assert int((rule & ((fall >> 12) - (k >> 12) >= 2)).sum()) >= (100 if strides > 3 else 10)
        for s in range(1, min(strides, 4)):                          # and first matches in each of strides 1 to 3
            assert int((needed & (k >> 12 == s)).sum()) >= 100, s


@pytest.mark.parametrize("name", ALL)
def test_host_form_against_the_rule_fields(name):
    rules = ns.shape(name)
    want = ns.host(name)
    some = ns.sample(rules, want)
    strides = (len(rules) + ns.STRIDE - 1) // ns.STRIDE
    assert len(some) == 64 and len(set(some)) == 64
    assert set(want["need"][some].tolist()) == {ns.DEAD, ns.REDUNDANT, ns.NEEDED}
    narrow_strides = set((ns.narrow(rules) >> 12).tolist())
    assert set(x >> 12 for x in some) == narrow_strides and len(narrow_strides) >= strides - 1
    for x in some:
        got = (int(want["first"][x]), int(want["changed"][x]), int(want["need"][x]), tuple(want["witness"][x].tolist()))
        assert got == ns.literal_for_rule(rules, x), x


def test_skip_sets():
    """The two skip sets of the GPU tests: a third of the rules, and the free
    rules (the second round); the second round changes need values."""
    for name in ("b", "g"):
        r = len(ns.shape(name))
        third = ns.skip_third(name)
        assert r // 4 < len(third) < r // 2
        a = ns.host(name, third, "third")
        assert a["counts"][ns.SKIPPED] == len(third) and a["counts"][ns.NEEDED] >= 100
        free = np.flatnonzero(ns.host(name)["free"]).tolist()
        b = ns.host(name, free, "free")
        assert b["counts"][ns.SKIPPED] == len(free)
        kept = np.setdiff1d(np.arange(r), free)
        assert int((b["need"][kept] != ns.host(name)["need"][kept]).sum()) >= 10
