"""Concurrent callers of the C ABI (tests/test_gpu_threads.py): the runner
and the checkers, free of the GPU so that tests/test_thread_cases_cpu.py can
show on fakes that they reject what they should.

``run_threads(fns, deadline_s)`` starts one daemon thread per callable behind
a barrier, so that all enter the library together, and re-raises the first
exception of any of them in the caller.  A thread that misses the deadline is
stuck inside a library call: the call cannot be interrupted and may hold an
engine mutex, so the runner does not return.  It dumps every Python stack,
takes the handles from the engines it was given (no fixture calls into them
again) and ends the pytest session with status 3 -- nothing more starts on the
GPU after a hang.  The deadline is a cap, never a measurement.

The checkers are plain numpy: ``one_of`` (a whole array equals exactly one
candidate: what a reader may see while a writer toggles between states) and
``sums_to``.
"""
import faulthandler
import functools
import sys
import threading
import time

import numpy as np

T = 8                   # threads per scenario (a GPU command has 16 CPUs)
DEADLINE_S = 120.0      # the cap of every scenario
EXIT_HANG = 3
MIN_SHARE = 0.05        # churn_case: the cells in which its two states differ, at least


def _dump(deadline_s, stuck):
    sys.stderr.write("run_threads: %d thread(s) still running after %.0f s: %s\n"
                     % (len(stuck), deadline_s, ", ".join(stuck)))
    faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
    sys.stderr.flush()


def _hang(engines, deadline_s, stuck, capture=None):
    """capture: the test's capfd / capsys fixture.  The session ends without
    showing what pytest captured, so the dump is written with the capture
    disabled and reaches the real stderr."""
    import pytest
    if capture is not None:
        with capture.disabled():
            _dump(deadline_s, stuck)
    else:
        _dump(deadline_s, stuck)
    # no handle is left to call the library with as the test's frames unwind:
    # a batch's destructor would take the engine mutex the stuck thread may hold
    for e in engines:
        for b in list(getattr(e, "_batches", ())):
            b.h = None
        for v in getattr(e, "_views", ()):
            for b in list(getattr(v, "_batches", ())):
                b.h = None
            v.h = None
        e.h = None
    pytest.exit("a thread is stuck in a library call; nothing more may run on the GPU", returncode=EXIT_HANG)


def run_threads(fns, deadline_s=DEADLINE_S, engines=(), capture=None):
    """Run the callables concurrently; returns their results in order.
    capture: the test's capfd or capsys fixture, for the stack dump of a hang."""
    fns = list(fns)
    barrier = threading.Barrier(len(fns))
    results = [None] * len(fns)
    errors = [None] * len(fns)

    def body(i, fn):
        try:
            barrier.wait(deadline_s)
            results[i] = fn()
        except BaseException as ex:          # re-raised in the caller
            errors[i] = ex
            barrier.abort()

    threads = [threading.Thread(target=body, args=(i, fn), name="caller%d" % i, daemon=True)
               for i, fn in enumerate(fns)]
    end = time.monotonic() + deadline_s
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, end - time.monotonic()))
    stuck = [t.name for t in threads if t.is_alive()]
    if stuck:
        _hang(engines, deadline_s, stuck, capture)
    # a thread's own failure before the BrokenBarrierError it caused in the others
    errs = [e for e in errors if e is not None]
    own = [e for e in errs if not isinstance(e, threading.BrokenBarrierError)]
    if own or errs:
        raise (own or errs)[0]
    return results


def one_of(got, candidates) -> int:
    """The index of the one candidate the whole array equals; AssertionError
    when it equals none of them (a mix of two states) or more than one (the
    candidates cannot tell the states apart)."""
    got = np.asarray(got)
    hit = [i for i, c in enumerate(candidates)
           if np.asarray(c).shape == got.shape and np.array_equal(got, np.asarray(c))]
    if len(hit) == 1:
        return hit[0]
    if not hit:
        near = []
        for c in candidates:
            c = np.asarray(c)
            near.append(int((got != c).sum()) if c.shape == got.shape else -1)
        raise AssertionError("equals no candidate: %s cells differ from each of them" % near)
    raise AssertionError("equals candidates %s: they are not distinct" % hit)


def sums_to(total, parts):
    """``total`` equals the element-wise sum of ``parts``, exactly (uint64)."""
    total = np.asarray(total).astype(np.uint64)
    acc = np.zeros(total.shape, np.uint64)
    for p in parts:
        p = np.asarray(p)
        assert p.shape == total.shape, (p.shape, total.shape)
        acc += p.astype(np.uint64)
    bad = np.nonzero(acc != total)
    assert len(bad[0]) == 0, "sum differs at %s: %s against %s" % (
        [b[:8].tolist() for b in bad], total[bad][:8].tolist(), acc[bad][:8].tolist())


def deny_any():
    """A rule without a protocol section and with empty networks: DENY for
    every packet."""
    from vpp_amd import model as M
    return M.Rule(actions=M.Actions(M.DENY), matches=M.Matches(ip_rule=M.IpRule(ip=M.Ip("", ""))))


def lib_reach_tile(value: int) -> int:
    """The tile the library makes of the option reach_tile=value: rounded up
    to a multiple of 1024 (options.cpp)."""
    return (value + 1023) & ~1023


def tiles(cells: int, reach_tile: int) -> int:
    """Tiles of a cls_reach_matrix call over `cells` cells."""
    t = lib_reach_tile(reach_tile)
    return -(-cells // t)


def churn_probes(c):
    """Twelve probes: 12 x 37 x 37 = 16,428 cells, which the smallest tile
    (1024 connections) cuts into 17.  The case's three, each four times under
    other source ports: probes on other destination ports are denied under R0
    and R1 alike by most of the case's ACLs and would thin the share of cells
    in which the two states differ to 2 %."""
    k = np.arange(12)
    return c["pr"][k % 3], (c["sp"][k % 3] + np.where(c["pr"][k % 3] < 2, k // 3, 0)).astype(np.uint16), c["dp"][k % 3]


@functools.lru_cache(maxsize=None)
def churn_case(fam):
    """reach_cases.case(fam) with one local ACL toggled between two rule
    lists: R0, its own, and R1 = deny-any + R0.  The ACL is the local one
    bound to the interface that carries the most endpoints -- the first, in
    that order, whose toggle changes at least MIN_SHARE of the matrix (the
    IPv4 case's first candidate changes 2.7 %: a reader that mixed two such
    states would have few cells to show it in).  Returns the ACL's name, its
    (ingress, egress) interfaces, R0, R1 and the oracle's matrices want0 (the
    case's) and want1 of the case's three probes, and big0 / big1 of the
    twelve probes pr, sp, dp (churn_probes), all read-only."""
    import reach_cases as rc
    from test_gpu_connect_scale import oracle_connections
    c = rc.case(fam)
    load = np.bincount(c["at"], minlength=len(c["ifs"]))
    tried = []
    for i in np.argsort(-load, kind="stable"):
        for name in c["bind"][c["ifs"][i]]:
            if name is None or name == "global" or name in tried:
                continue
            tried.append(name)
            r0 = list(c["by_name"][name])
            r1 = [deny_any()] + r0
            by_name = dict(c["by_name"])
            by_name[name] = r1
            want1, _ = oracle_connections(c["bind"], by_name, c["ifs"], c["si"], c["di"], c["tr"], fam)
            want1 = want1.reshape(c["want"].shape)
            if differing_share(c["want"], want1) < MIN_SHARE:
                continue
            want1.setflags(write=False)
            ing = [i for i in c["ifs"] if c["bind"][i][0] == name]
            eg = [i for i in c["ifs"] if c["bind"][i][1] == name]
            # the matrix readers' probes: the case's three first, then nine more
            pr, sp, dp = churn_probes(c)
            si, di, tr = rc.expand(c["at"], c["addrs"], pr, sp, dp)
            big = []
            for rules in (c["by_name"], by_name):
                w, _ = oracle_connections(c["bind"], rules, c["ifs"], si, di, tr, fam)
                w = w.reshape(len(pr), len(c["at"]), len(c["at"]))
                w.setflags(write=False)
                big.append(w)
            assert np.array_equal(big[0][:3], c["want"]) and np.array_equal(big[1][:3], want1)
            return dict(name=name, ing=ing, eg=eg, r0=r0, r1=r1, want0=c["want"], want1=want1,
                        pr=pr, sp=sp, dp=dp, big0=big[0], big1=big[1])
    raise AssertionError("no local ACL's toggle changes %.0f %% of the matrix" % (100 * MIN_SHARE))


def differing_share(a, b) -> float:
    """The share of cells in which two equal-shaped arrays differ."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    return float((a != b).mean())
