"""The reachability-diff tests' shared case (tests/test_gpu_reach_diff.py,
tests/test_reach_diff_cpu.py): reach_cases.case(fam) -- 37 endpoints x 3
probes = 4,107 cells, no multiple of 4, 64 or 1024 -- before and after a real
ACL change: `local4` deleted (its interfaces lose the binding; a nil ACL is
PERMIT) and `local9` re-put with other rules on the interfaces that bind it.
The expected matrices are the C oracle's, computed once per family and never
modified; diff_ref is the numpy definition of what cls_reach_diff reports."""
import functools

import numpy as np

import reach_cases as rc

DELETED, REPUT = "local4", "local9"


def _reput_rules(fam):
    from aclgen import random_acl, random_acl16
    return (random_acl16 if fam == 16 else random_acl)(7001, 40, weird=0.0)[0]


def _bound(bind, ifs, name):
    """(ingress, egress) interfaces that bind an ACL."""
    return [i for i in ifs if bind[i][0] == name], [i for i in ifs if bind[i][1] == name]


@functools.lru_cache(maxsize=None)
def after(fam):
    """The case after the change: its bind and by_name, the oracle's matrix
    (read-only) and counters."""
    from test_gpu_connect_scale import oracle_connections
    c = rc.case(fam)
    bind = {i: [None if x == DELETED else x for x in b] for i, b in c["bind"].items()}
    by_name = {k: v for k, v in c["by_name"].items() if k != DELETED}
    assert any(DELETED in b for b in c["bind"].values()) and any(REPUT in b for b in c["bind"].values())
    by_name[REPUT] = _reput_rules(fam)
    want, counts = oracle_connections(bind, by_name, c["ifs"], c["si"], c["di"], c["tr"], fam)
    want = want.reshape(c["want"].shape)
    want.setflags(write=False)
    return dict(c, bind=bind, by_name=by_name, want=want, counts=counts)


def apply(eng, c):
    """The same two edits on an engine that has the case installed."""
    assert eng.acl_del(DELETED) == 0
    ing, eg = _bound(c["bind"], c["ifs"], REPUT)
    assert eng.acl_put(REPUT, _reput_rules(c["fam"]), ing, eg) == 0


def records(cells, base, new, n):
    """The record array of flat cell indices of a [P, N, N] pair."""
    from vpp_amd import _abi
    out = np.zeros(len(cells), _abi.REACH_CHANGE)
    out["probe"], out["src"], out["dst"] = cells // (n * n), cells // n % n, cells % n
    out["was"], out["now"] = base.ravel()[cells], new.ravel()[cells]
    return out


def diff_ref(base, new, cap=None):
    """What cls_reach_diff reports of base -> new ([P, N, N] u8 each): the
    changed cells' records in flatnonzero order (the first cap), their total,
    trans [P, 4, 4] u64 (cells per (base & 3, new)) and changed [P, N] u32."""
    base, new = np.asarray(base, np.uint8), np.asarray(new, np.uint8)
    P, N = base.shape[0], base.shape[1]
    cells = np.flatnonzero(base.ravel() != new.ravel())
    total = len(cells)
    trans = np.zeros((P, 4, 4), np.uint64)
    for p in range(P):
        np.add.at(trans[p], ((base[p] & 3).ravel(), new[p].ravel()), 1)
    changed = (base != new).sum(axis=2).astype(np.uint32)
    return records(cells[:total if cap is None else cap], base, new, N), total, trans, changed
