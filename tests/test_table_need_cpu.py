"""The rule necessity sweep without a GPU: cls_table_need_host (the definition
in plain C++ over the bit rows) against need_cases.need_ref (the oracle over
the cells), the reference's shortcut pinned to the literal definition on small
tables, the named expectations of the constructed ACLs, skip, the Python round
loop on the host form, and the agreement of header, binding and library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cover_cases as cc
import need_cases as nc
from aclgen import random_acl
from vpp_amd import _abi
from vpp_amd.engine import Engine, minimize_rounds, v6_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 63, 64, 65, 130]


def random_table(n):
    """aclgen.random_acl of n rules, malformed ones included, below 2^16 cells."""
    rules = random_acl(n * 5 + 3, n, 0.3, n_prefixes=5)[0]
    assert cc.dims(rules)[1] <= nc.MAX_CELLS, cc.dims(rules)
    return rules


# ---- the reference's shortcut against the literal definition ---------------------

@pytest.mark.parametrize("table", ["need_acl", "need_acl_fail", "random1", "random30"])
def test_reference_shortcut_is_the_literal_definition(table):
    rules = {"need_acl": nc.need_acl, "need_acl_fail": nc.need_acl_fail, "random1": lambda: random_table(1),
             "random30": lambda: random_table(30)}[table]()
    want = nc.ref(table, rules)
    lit = nc.need_literal(rules)
    for k, (n_diff, least) in enumerate(lit):
        assert (want["need"][k] == nc.NEEDED) == (n_diff > 0), k
        assert int(want["changed"][k]) == n_diff, k
        assert tuple(want["witness"][k]) == (least or (0, 0, 0, 0, 0, 0)), k


# ---- the host form against the reference ------------------------------------------

def test_need_acl_named_expectations():
    rules = nc.need_acl()
    at = nc.names(rules).index
    got = Engine.table_need_host(rules)
    nc.assert_equal(got, nc.ref("need_acl", rules), "need_acl")
    need, free, w, r = got["need"], got["free"], got["witness"], len(rules)

    def ip(a, b, c, d):
        return a << 24 | b << 16 | c << 8 | d
    assert need[at("deny_udp")] == nc.REDUNDANT and free[at("deny_udp")] == 1
    assert need[at("deny_tcp")] == nc.REDUNDANT and free[at("deny_tcp")] == 0
    assert need[at("a32")] == nc.REDUNDANT and free[at("a32")] == 1 and need[at("a24")] == nc.NEEDED
    assert need[at("b32")] == nc.NEEDED
    assert tuple(w[at("b32")]) == (ip(10, 1, 0, 5), 0, 80, 0, 0x80 | 0, at("bdeny"))
    assert need[at("c24")] == nc.DEAD and free[at("c24")] == 1
    assert need[at("d1")] == nc.REDUNDANT and free[at("d1")] == 0
    assert need[at("d2")] == nc.DEAD and free[at("d2")] == 1
    assert need[at("e1")] == nc.NEEDED and w[at("e1")]["after"] == 0x80 | 2 and w[at("e1")]["fall"] == at("e2")
    assert need[at("f1")] == nc.NEEDED and w[at("f1")]["after"] == 0x80 | 1 and w[at("f1")]["fall"] == at("f2")
    assert need[at("g")] == nc.NEEDED and w[at("g")]["proto"] == 3
    assert need[at("v6")] == nc.DEAD
    assert got["counts"].sum() == r and got["counts"][nc.SKIPPED] == 0
    # after one round d1 is NEEDED, and deny_tcp falls to the default alone
    gone = [k for k in range(r) if free[k]]
    again = Engine.table_need_host(rules, skip=gone)
    nc.assert_equal(again, nc.ref("need_acl", rules, gone), "need_acl, second round")
    assert again["need"][at("d1")] == nc.NEEDED
    assert again["need"][at("deny_tcp")] == nc.REDUNDANT and again["free"][at("deny_tcp")] == 1
    assert all(again["need"][k] == nc.SKIPPED for k in gone)


def test_unconditional_failure_makes_everything_behind_it_dead():
    rules = nc.need_acl_fail()
    at = nc.names(rules).index
    got = Engine.table_need_host(rules)
    nc.assert_equal(got, nc.ref("need_acl_fail", rules), "need_acl_fail")
    assert got["need"].tolist() == [nc.NEEDED, nc.NEEDED, nc.DEAD, nc.DEAD]
    # what is behind the FAILURE takes over once it is gone: the least packet falls to after_a
    w = got["witness"][at("macip")]
    assert (w["src"], w["dst"], w["proto"], w["dport"]) == (0, 0, 0, 0)
    assert w["after"] == 0x80 | 1 and w["fall"] == at("after_a")
    assert got["first"][len(rules)] == 0


@pytest.mark.parametrize("n", SIZES)
def test_host_random(n):
    rules = random_table(n)
    got = Engine.table_need_host(rules)
    nc.assert_equal(got, nc.ref("random%d" % n, rules), "random %d" % n)
    assert len(got["need"]) == n


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_host_skip(n):
    """Skipping {r} equals the sweep of the list without r, indices shifted
    (need, free and the witnesses are canonical; the cell counts are relative
    to the longer list's classes); skipping everything leaves the default."""
    rules = random_table(n)
    rng = np.random.default_rng(n)
    for r in sorted(set(int(x) for x in rng.integers(0, n, 4)) | {0, n - 1}):
        got = Engine.table_need_host(rules, skip=[r])
        nc.assert_equal(got, nc.ref("random%d" % n, rules, [r]), "random %d skip %d" % (n, r))
        short = Engine.table_need_host(rules[:r] + rules[r + 1:])
        keep = np.arange(n) != r
        assert got["need"][r] == nc.SKIPPED and got["free"][r] == 0 and got["changed"][r] == 0
        assert np.array_equal(got["need"][keep], short["need"]) and np.array_equal(got["free"][keep], short["free"])
        w = short["witness"].copy()
        up = (w["after"] != 0) & (w["fall"] >= r)
        w["fall"][up] += 1
        assert got["witness"][keep].tobytes() == w.tobytes()
        assert tuple(got["witness"][r]) == (0, 0, 0, 0, 0, 0)
    got = Engine.table_need_host(rules, skip=range(n))
    assert np.all(got["need"] == nc.SKIPPED) and not got["free"].any() and not got["changed"].any()
    assert got["first"][n] == got["n_cells"] and got["counts"].tolist() == [n, 0, 0, 0]
    assert got["witness"].tobytes() == bytes(16 * n)


def test_host_strided_words():
    """W = 66: the placed first and second matches across words 0, 63 and 64."""
    rules = nc.strided_acl()
    at = nc.names(rules).index
    got = Engine.table_need_host(rules)
    nc.assert_equal(got, nc.ref("strided", rules), "strided")
    w = got["witness"]
    assert (at("w0a"), at("w0b"), at("w0_64a"), at("w0_64b"), at("w63_64a"), at("w63_64b")) == (0, 1, 2, 4100, 4040, 4110)
    assert w[0]["fall"] == 1 and w[2]["fall"] == 4100
    assert got["need"][4040] == nc.REDUNDANT and got["free"][4040] == 0 and got["need"][4110] == nc.DEAD
    assert got["need"][3] == nc.NEEDED and w[3]["fall"] == len(rules)
    assert got["first"][len(rules)] > 0


def test_host_refusals():
    L = _abi.lib()
    rules = random_table(30)
    cr = _abi.CRules(rules)
    need = np.full(30, 0xA5, np.uint8)
    o = _abi.NeedOut(need.ctypes.data, None, None, None, None, None, None, None)
    assert L.cls_table_need_host(cr.ptr(), cr.n, None, None) == _abi.E_INVAL
    assert L.cls_table_need_host(cr.ptr(), cr.n, None, C.byref(_abi.NeedOut())) == _abi.E_INVAL
    assert L.cls_table_need_host(None, 3, None, C.byref(o)) == _abi.E_INVAL
    assert np.all(need == 0xA5)
    assert L.cls_table_need_host(cr.ptr(), cr.n, None, C.byref(o)) == 0
    assert np.array_equal(need, nc.ref("random30", rules)["need"])
    # only n_cells and dims: no output
    n_cells = np.zeros(1, np.uint64)
    o = _abi.NeedOut(None, None, None, None, None, None, n_cells.ctypes.data, None)
    assert L.cls_table_need_host(cr.ptr(), cr.n, None, C.byref(o)) == _abi.E_INVAL


# ---- the round loop -----------------------------------------------------------------

def _rounds(rules, keep=(), **kw):
    return minimize_rounds(lambda skip: Engine.table_need_host(rules, skip=skip), len(rules), keep, **kw)


def test_round_loop_on_the_host_form():
    rules = nc.need_acl()
    at = nc.names(rules).index
    pinned = v6_rules(rules)
    assert pinned == [at("v6")]
    kept, rounds = _rounds(rules, pinned)
    assert len(rounds) == 2 and at("d2") in rounds[0] and at("deny_udp") in rounds[0]
    assert at("deny_tcp") in rounds[1] and at("d1") in kept and at("v6") in kept
    removed = [k for r in rounds for k in r]
    assert sorted(kept + removed) == list(range(len(rules)))
    # the result's own sweep: nothing dead or redundant outside keep
    last = Engine.table_need_host(rules, skip=removed)
    loose = [k for k in kept if last["need"][k] in (nc.DEAD, nc.REDUNDANT)]
    assert loose == pinned
    # and the reduced list gives every cell of the original list the same action
    c = cc.cells(rules)
    full = nc._classify(nc.oracle.rules_to_c(rules), np.arange(len(rules)), len(rules), c)[0]
    less = nc._classify(nc.oracle.rules_to_c(rules), np.array(kept), len(rules), c)[0]
    assert np.array_equal(full, less)
    # without the pin the IPv6 rule goes in the first round; max_rounds cuts the loop short
    kept2, rounds2 = _rounds(rules)
    assert at("v6") in rounds2[0] and at("v6") not in kept2
    kept1, rounds1 = _rounds(rules, pinned, max_rounds=1)
    assert rounds1 == rounds[:1] and at("deny_tcp") in kept1


@pytest.mark.parametrize("n", [65, 130])
def test_round_loop_random(n):
    rules = random_table(n)
    kept, rounds = _rounds(rules)
    removed = [k for r in rounds for k in r]
    want = nc.ref("random%d" % n, rules)
    assert (len(rounds) > 0) == bool(((want["need"] == nc.DEAD) | (want["need"] == nc.REDUNDANT)).any())
    last = Engine.table_need_host(rules, skip=removed)
    assert all(last["need"][k] == nc.NEEDED for k in kept)
    c = cc.cells(rules)
    cr = nc.oracle.rules_to_c(rules)
    assert np.array_equal(nc._classify(cr, np.arange(n), n, c)[0], nc._classify(cr, np.array(kept, np.int64), n, c)[0])


# ---- header, binding, library -------------------------------------------------------

def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", "contivcls.h")).read()
    for sym in ("cls_table_need", "cls_table_need_host"):
        assert sym in _abi.SYMBOLS and hasattr(_abi.lib(), sym)
        assert re.search(r"^int %s\(" % sym, text, re.M), sym
    vals = dict(re.findall(r"CLS_NEED_(\w+) = (\d)", text))
    assert vals == {"SKIPPED": str(_abi.NEED_SKIPPED), "DEAD": str(_abi.NEED_DEAD),
                    "REDUNDANT": str(_abi.NEED_REDUNDANT), "NEEDED": str(_abi.NEED_NEEDED)}
    assert _abi.NEED_WITNESS.itemsize == 16 and _abi.NEED_WITNESS.names == ("src", "dst", "dport", "proto", "after", "fall")
    body = re.search(r"typedef struct cls_need_out \{(.*?)\} cls_need_out;", text, re.S).group(1)
    fields = re.findall(r"\*\s*(\w+);", body)
    assert fields == [f for f, _ in _abi.NeedOut._fields_]
    assert _abi.lib().cls_abi_version() == 5
