"""GPU: the C ABI's threading contract (include/contivcls.h, INTEGRATION.md
"Threading and ownership") under concurrent callers.

Eight Python threads call one engine through ctypes, which releases the GIL,
so they meet inside the library: at its mutex, on its shared host staging and
scratch, its per-(table, stream) counter scratch, the connection plan and its
conn_last / conn_sync_ev ordering, the reach scratch, the timing event pool,
the generator pools, the peers' locks of a multi-device engine.  Every oracle
result is computed before the threads start, and so is every output that is
filled with a sentinel or zeros (a torch fill runs on torch's own stream, not
on the caller's); the reach calls' outputs are allocated uninitialised
(torch.empty, no device work) by the Engine methods inside the threads.  The
threads only call the library, and the main thread compares afterwards, bit
for bit.  The only expected outcome anywhere is
"equal to the oracle"; under concurrency the tests go by return codes, never
by cls_last_error's text.

The tests only add callers: what they can show of a race on the GPU is
probabilistic.  Deterministic are the checkers (test_thread_cases_cpu.py),
the atomicity invariant of the ACL churn (a reader sees one of two whole
states), and the exact totals of the timing pool and the connection counters.
A thread that does not come back ends the session (thread_cases.run_threads).
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import oracle
import reach_cases as rc
import reach_diff_cases as dc
import reach_hops_cases as hc
import reach_ports_cases as pc
import thread_cases as tc
from aclgen import random_acl, random_acl16, random_traffic, random_traffic16, single_port_acl
from vpp_amd import _abi

pytestmark = pytest.mark.gpu

T = tc.T
K = 10                   # calls per thread
N = 40003                # packets per classify batch: odd, 10 workgroups
R = 400
OTHER = 0.125            # protocol 47: the OTHER queue and the finish launch run
GATE_S = 60.0            # a barrier inside a scenario: broken well before the scenario's deadline


CAPTURE = []             # the running test's capfd: a hang's stack dump goes past it to the real stderr


@pytest.fixture(autouse=True)
def _capture(capfd):
    CAPTURE[:] = [capfd]
    yield
    CAPTURE.clear()


def _engine(**kw):
    from vpp_amd.engine import Engine
    return Engine(**kw)


def _run(fns, *engines):
    return tc.run_threads(fns, tc.DEADLINE_S, engines, CAPTURE[0] if CAPTURE else None)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (what, bad.size, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


def _dev(x):
    """A host array as a torch GPU tensor of the same bytes (its own
    allocation: aligned as the vector paths want)."""
    import torch
    x = np.array(x, order="C")          # a writable copy: the shared cases are read-only
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(x.view(signed.get(x.dtype, x.dtype))).cuda()


def _np(t, dtype):
    return t.cpu().numpy().view(dtype)


def _sync():
    import torch
    torch.cuda.synchronize()


def _streams(n):
    import torch
    return [torch.cuda.Stream() for _ in range(n)]


# ---- the classify case -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _acl_and_packets(af):
    """The 400-rule random ACL and 2 N packets aimed at its prefixes."""
    v16 = af == 16
    rules, pool = (random_acl16 if v16 else random_acl)(417, R, 0.05)
    return rules, (random_traffic16 if v16 else random_traffic)(30, 2 * N, pool)


@functools.lru_cache(maxsize=None)
def classify_case(af, n=N, n_batches=T):
    """(rules, [(batch, verdicts, rules hit, counters)] x n_batches): a
    400-rule random ACL and batches drawn under different seeds (each its own
    sample, with repeats, of the ACL's packets -- drawing 16-byte packets
    afresh takes most of a second per batch), an eighth of each protocol 47,
    with the oracle's results; read-only."""
    rules, packets = _acl_and_packets(af)
    cr = oracle.rules_to_c(rules)
    out = []
    for i in range(n_batches):
        rng = np.random.default_rng(900 + i)
        at = rng.integers(0, 2 * N, n)
        tr = {k: np.ascontiguousarray(packets[k][at]) for k in ("src", "dst", "dport", "proto")}
        tr["proto"] = np.where(rng.random(n) < OTHER, 47, tr["proto"]).astype(np.uint8)
        ov, oh = oracle.classify_hits(cr, tr["src"], tr["dst"], tr["dport"], tr["proto"], af=af)
        oc = np.bincount(oh, minlength=len(rules) + 1).astype(np.uint64)
        assert (tr["proto"] == 47).sum() > n // 10 and len(np.unique(ov)) >= 2
        for a in list(tr.values()) + [ov, oh, oc]:
            a.setflags(write=False)
        out.append((tr, ov, oh, oc))
    return rules, out


def _to_device(tr):
    return {k: _dev(tr[k]) for k in ("src", "dst", "dport", "proto")}


class Outs:
    """The outputs of `k` device classify calls, allocated and filled before
    the threads start: even calls are cls_classify (verdicts + counters), odd
    ones cls_classify_rules (verdicts + rules)."""

    def __init__(self, k, n, n_rules):
        import torch
        self.v = [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(k)]
        self.c = [torch.zeros(n_rules + 1, dtype=torch.int64, device="cuda") for _ in range(k)]
        self.r = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(k)]

    def check(self, want, what, timing=False):
        _, ov, oh, oc = want
        for j in range(len(self.v)):
            _same(_np(self.v[j], np.uint8), ov, "%s call %d: verdicts" % (what, j))
            if j & 1 and not timing:
                _same(_np(self.r[j], np.uint32), oh, "%s call %d: rules" % (what, j))
            else:
                _same(_np(self.c[j], np.uint64), oc, "%s call %d: counters" % (what, j))


def _classify_calls(eng, t, d, outs, stream, k=K, timing=False, each=None):
    """k device calls on `stream` (0: the engine's), alternating cls_classify
    and cls_classify_rules (timing: cls_classify with CLS_F_TIMING alone)."""
    for j in range(k):
        if j & 1 and not timing:
            eng.classify_rules(t, d["src"], d["dst"], d["dport"], d["proto"], verdict=outs.v[j], rules=outs.r[j],
                               stream=stream)
        else:
            eng.classify(t, d["src"], d["dst"], d["dport"], d["proto"], verdict=outs.v[j], counters=outs.c[j],
                         timing=timing, stream=stream)
        if each is not None:
            each(j)


def _host_calls(eng, t, want, what, k=K):
    """k host-array calls, checked as they return."""
    tr, ov, oh, oc = want
    for j in range(k):
        if j & 1:
            v, r = eng.classify_rules(t, tr["src"], tr["dst"], tr["dport"], tr["proto"])
            _same(r, oh, "%s call %d: rules" % (what, j))
        else:
            v, c = eng.classify(t, tr["src"], tr["dst"], tr["dport"], tr["proto"])
            _same(c, oc, "%s call %d: counters" % (what, j))
        _same(v, ov, "%s call %d: verdicts" % (what, j))


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


# ---- 1: classify, one table, many callers -------------------------------------

@pytest.mark.parametrize("variant", ["own_stream", "engine_stream", "host"])
@pytest.mark.parametrize("af", [4, 16])
def test_classify_one_table_many_callers(eng, af, variant):
    """Shared: the engine mutex, the table's per-(table, stream) counter
    scratch and OTHER queue (own_stream: eight scratches; engine_stream: one,
    stream-ordered), the host staging s_src .. s_rule (host)."""
    rules, batches = classify_case(af)
    t = eng.put_table("many", rules)
    try:
        if variant == "host":
            _run([lambda i=i: _host_calls(eng, t, batches[i], "thread %d" % i) for i in range(T)], eng)
            return
        devs = [_to_device(b[0]) for b in batches]
        outs = [Outs(K, N, len(rules)) for _ in range(T)]
        streams = _streams(T) if variant == "own_stream" else [0] * T
        _sync()
        _run([lambda i=i: _classify_calls(eng, t, devs[i], outs[i], streams[i]) for i in range(T)], eng)
        _sync()
        for i in range(T):
            outs[i].check(batches[i], "thread %d" % i)
    finally:
        if eng.h:
            eng.del_table(t)


@pytest.mark.parametrize("af", [4, 16])
def test_classify_lds_and_global_image_tables(eng, af):
    """Half the callers on table A (image in LDS), half on table B of the
    same rules compiled under lds_budget=256 (image in global memory), the
    option back at its default before the threads start."""
    rules, batches = classify_case(af)
    a = eng.put_table("A", rules)
    eng.set_option("lds_budget", 256)
    try:
        b = eng.put_table("B", rules)
    finally:
        eng.set_option("lds_budget", None)
    try:
        res = "lds_resident_v16" if af == 16 else "lds_resident"
        assert a.info()[res] == 1 and b.info()[res] == 0
        devs = [_to_device(x[0]) for x in batches]
        outs = [Outs(K, N, len(rules)) for _ in range(T)]
        streams = _streams(T)
        _sync()
        _run([lambda i=i: _classify_calls(eng, (a, b)[i & 1], devs[i], outs[i], streams[i]) for i in range(T)], eng)
        _sync()
        for i in range(T):
            outs[i].check(batches[i], "thread %d (table %s)" % (i, "AB"[i & 1]))
    finally:
        if eng.h:
            eng.del_table(a)
            eng.del_table(b)


# ---- 2: timing ----------------------------------------------------------------

def _stall(stream):
    """Device work of some tens of milliseconds on `stream`: what is enqueued
    behind it is still pending when the next host calls are made (the callers
    check that with an event)."""
    import torch
    with torch.cuda.stream(stream):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(100_000_000)
        else:
            a = torch.ones((4096, 4096), device="cuda")
            for _ in range(20):
                a = (a @ a).clamp_(0, 1)


@pytest.mark.parametrize("variant", ["engine_stream", "own_stream"])
@pytest.mark.parametrize("af", [4, 16])
def test_timing_pool_and_last_kernel_ms(eng, af, variant):
    """CLS_F_TIMING from eight threads while each reads cls_last_kernel_ms:
    the event pool (ev_pool / ev_used) and the last pair (ev0 / ev1, timed).
    cls_last_kernel_ms takes the engine mutex like its siblings: every call is
    CLS_OK with a finite time > 0 -- never a pair handed out and not yet
    recorded, never the start of one call with the end of another.  The pool
    then holds exactly T K entries, in launch order.  On the engine's stream
    launch order is start order, so cls_kernel_starts is non-decreasing from
    0: a pair handed to two calls or an entry out of place would break it.
    Across eight streams the hardware starts kernels of different queues in
    any order (a later launch on an idle queue overtakes one behind its
    stream's backlog), so there the order of the starts is no property of the
    library and is not asserted; the count and the durations are."""
    L = _abi.lib()
    rules, batches = classify_case(af)
    t = eng.put_table("timed", rules)
    try:
        eng.kernel_times(reset=True)
        devs = [_to_device(b[0]) for b in batches]
        outs = [Outs(K, N, len(rules)) for _ in range(T)]
        streams = _streams(T) if variant == "own_stream" else [0] * T
        seen = [[] for _ in range(T)]
        _sync()

        def caller(i):
            def read(_j):
                ms = C.c_float(float("nan"))
                seen[i].append((L.cls_last_kernel_ms(eng.h, C.byref(ms)), ms.value))
            _classify_calls(eng, t, devs[i], outs[i], streams[i], timing=True, each=read)
        _run([lambda i=i: caller(i) for i in range(T)], eng)
        # read with no device synchronise in front: the call itself waits for every pair
        times, starts = eng.kernel_times(reset=True, starts=True)
        _sync()
        for i in range(T):
            assert len(seen[i]) == K
            for rc_, ms in seen[i]:
                assert rc_ == _abi.OK and np.isfinite(ms) and ms > 0, (i, seen[i])
            outs[i].check(batches[i], "thread %d" % i, timing=True)
        print("timing af %d %s: %d entries, durations %.4f .. %.4f ms, last start %.3f ms" % (
            af, variant, len(times), min(times), max(times), starts[-1]))
        assert len(times) == T * K and len(starts) == T * K
        assert all(np.isfinite(x) and x > 0 for x in times), times
        assert starts[0] == 0 and all(np.isfinite(x) for x in starts), starts
        if variant == "engine_stream":
            assert all(b >= a for a, b in zip(starts, starts[1:])), starts
    finally:
        if eng.h:
            eng.del_table(t)


@pytest.mark.parametrize("af", [4, 16])
def test_kernel_times_wait_for_every_stream(eng, af):
    """Two timed calls from one thread: the first on a stream still busy with
    a stall (checked with an event just before the read), the second -- the
    last pair of the pool -- on an idle stream.  cls_kernel_times, _starts and
    _reset wait for every pair's end: waiting for the last pair alone would
    leave the first one's events unrecorded when their times are read."""
    import torch
    rules, batches = classify_case(af)
    t = eng.put_table("two_streams", rules)
    try:
        eng.kernel_times(reset=True)
        devs = [_to_device(batches[i][0]) for i in range(2)]
        outs = [Outs(1, N, len(rules)) for _ in range(2)]
        streams = _streams(2)
        busy = torch.cuda.Event()
        _sync()
        _stall(streams[0])
        for i in range(2):
            _classify_calls(eng, t, devs[i], outs[i], streams[i], k=1, timing=True)
        busy.record(streams[0])
        pending = not busy.query()
        times, starts = eng.kernel_times(reset=False, starts=True)
        assert pending, "the stall ended before the pool was read: the premise is not met"
        assert len(times) == 2 and all(np.isfinite(x) and x > 0 for x in times), times
        assert starts[0] == 0 and np.isfinite(starts[1]), starts
        eng.kernel_times(reset=True)
        _sync()
        for i in range(2):
            outs[i].check(batches[i], "stream %d" % i, timing=True)
    finally:
        if eng.h:
            eng.del_table(t)


# ---- 3: table churn ------------------------------------------------------------

@pytest.mark.parametrize("af", [4, 16])
def test_table_churn(af):
    """Seven readers on table X while a writer puts, inspects and deletes
    other tables (9 .. 400 rules, one without a 16-byte classifier) and
    re-puts an equal ACL (a rebind): tables, next_table, conn_gen, the
    compiler.  The readers' K calls are paced by the writer, one per four of
    its rounds, so that reads and churn overlap throughout.  Then X is deleted
    while reader work is queued behind a stall on every reader stream (an
    event per stream, queried just before the delete, shows it still
    pending): its buffers are freed only after that work, every result is
    exact, and a reader's next call is CLS_E_NOTFOUND."""
    import torch
    from test_directed_traffic_cpu import refused_v16_table
    L = _abi.lib()
    n_read = T - 1
    rules, batches = classify_case(af)
    others = [random_acl(800 + k, size, 0.05)[0] for k, size in enumerate((9, 40, 150, 400))]
    others.append(refused_v16_table()[0])
    e = _engine()
    try:
        x = e.put_table("X", rules)
        assert e.acl_put("rebound", others[1], ["ifA"], ["ifB"]) == 0
        devs = [_to_device(b[0]) for b in batches[:n_read]]
        outs = [Outs(K, N, len(rules)) for _ in range(n_read)]
        late = [Outs(1, N, len(rules)) for _ in range(n_read)]
        streams = _streams(n_read)
        gate = threading.Barrier(T)
        ticks = [threading.Event() for _ in range(K)]      # tick j: the writer began round 4 j
        queued = [torch.cuda.Event() for _ in range(n_read)]
        pending = []
        after = [None] * n_read
        _sync()

        def guarded(fn):
            """A thread that fails releases the others from the gate."""
            def run(*a):
                try:
                    return fn(*a)
                except BaseException:
                    gate.abort()
                    for tick in ticks:
                        tick.set()
                    raise
            return run

        @guarded
        def reader(i):
            ticks[0].wait(GATE_S)
            _classify_calls(e, x, devs[i], outs[i], streams[i],
                            each=lambda j: j + 1 < K and ticks[j + 1].wait(GATE_S))
            gate.wait(GATE_S)                         # the writer's rounds are done
            _stall(streams[i])
            _classify_calls(e, x, devs[i], late[i], streams[i], k=1)
            queued[i].record(streams[i])
            gate.wait(GATE_S)                         # every reader's last call is queued
            gate.wait(GATE_S)                         # X is deleted
            d = devs[i]
            pk = _abi.PktSoa(af, *((None, None, d["src"].data_ptr(), d["dst"].data_ptr()) if af == 16 else
                                   (d["src"].data_ptr(), d["dst"].data_ptr(), None, None)), None,
                             d["dport"].data_ptr(), d["proto"].data_ptr())
            after[i] = L.cls_classify(e.h, x.id, C.byref(pk), N, late[i].v[0].data_ptr(), None, _abi.F_DEVICE,
                                      streams[i].cuda_stream)

        @guarded
        def writer():
            for k in range(40):
                if k % 4 == 0:
                    ticks[k // 4].set()
                t = e.put_table("other%d" % k, others[k % len(others)])
                info = t.info()
                assert info["n_rules"] == len(others[k % len(others)])
                if k % len(others) == 4:
                    assert info["has_v16"] == 0
                e.del_table(t)
                if k % 8 == 0:
                    assert e.acl_put("rebound", others[1], ["ifA"], ["ifB"]) == 0
            gate.wait(GATE_S)
            gate.wait(GATE_S)
            pending.extend(not ev.query() for ev in queued)
            rc_ = L.cls_table_del(e.h, x.id)
            gate.wait(GATE_S)
            assert rc_ == _abi.OK
        _run([lambda i=i: reader(i) for i in range(n_read)] + [writer], e)
        _sync()
        assert pending == [True] * n_read, "reader work had finished before the delete: %s" % pending
        assert after == [_abi.E_NOTFOUND] * n_read, after
        for i in range(n_read):
            outs[i].check(batches[i], "reader %d" % i)
            late[i].check(batches[i], "reader %d, queued at the delete" % i)
        assert e.acl_stats()[1] >= 5                   # the equal puts kept the table
    finally:
        e.close()


# ---- the connection / reach case on shared engines ------------------------------

@pytest.fixture(scope="module")
def installed():
    """Engines with reach_cases.case(fam) installed, made on first use:
    (engine, interface id per interface name index, per endpoint)."""
    made = {}

    def get(fam):
        if fam not in made:
            e = _engine()
            c = rc.case(fam)
            ep_ids = rc.install(e, c)
            if_ids = np.array([e.if_id(x) for x in c["ifs"]], np.uint32)
            made[fam] = (e, if_ids, ep_ids)
        return made[fam]
    yield get
    for e, _, _ in made.values():
        e.close()


@functools.lru_cache(maxsize=None)
def conn_rows(fam):
    """The case's rows as a connection batch's host arrays (interface indices,
    not ids), and the oracle's trace of them."""
    from test_connect_trace_cpu import oracle_rows
    c = rc.case(fam)
    v, rows = oracle_rows(c["bind"], c["by_name"], c["ifs"], c["si"], c["di"], c["tr"], fam)
    assert np.array_equal(v, c["want"].ravel())
    rows.setflags(write=False)
    return rows


def _conn_host(c, if_ids):
    tr = c["tr"]
    return [if_ids[c["si"]], if_ids[c["di"]], tr["src"], tr["dst"], tr["proto"], tr["sport"], tr["dport"]]


def _conn_soa(fam, d):
    """cls_conn_soa over the device tensors d = [sif, dif, src, dst, proto, sport, dport]."""
    p = [x.data_ptr() for x in d]
    if fam == 16:
        pk = _abi.PktSoa(_abi.AF_V16, None, None, p[2], p[3], p[5], p[6], p[4])
    else:
        pk = _abi.PktSoa(_abi.AF_V4, p[2], p[3], None, None, p[5], p[6], p[4])
    return _abi.ConnSoa(pk, p[0], p[1])


def _conn_outs(k, n):
    import torch
    return [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(k)]


# ---- 4: connection batches with counters ---------------------------------------

@pytest.mark.parametrize("fam", [4, 16])
def test_connection_batches_with_counters(installed, fam):
    """Six threads enqueue counted device batches on their own streams, two
    call with host arrays, one of the six also traces (cls_connect_rules):
    the connection scratch, the kept ConnPlan and up_*, conn_last /
    conn_sync_ev, the tables' counter rows and scatter events.  Verdicts and
    the trace are exact; the counters, read once with reset, are exactly T K
    times the oracle's, and all zero afterwards."""
    import torch
    L = _abi.lib()
    e, if_ids, _ = installed(fam)
    c = rc.case(fam)
    want, rows = c["want"].ravel(), conn_rows(fam)
    n = len(want)
    host = _conn_host(c, if_ids)
    d = [_dev(x) for x in host]
    cs = _conn_soa(fam, d)
    n_dev = T - 2
    outs = [_conn_outs(K, n) for _ in range(n_dev)]
    tv = _conn_outs(K, n)
    tr_out = [torch.full((n, 4), -7, dtype=torch.int32, device="cuda") for _ in range(K)]
    streams = _streams(n_dev)
    for name in c["by_name"]:
        e.conn_counters(name, reset=True)
    _sync()

    def device(i):
        s = streams[i].cuda_stream
        for j in range(K):
            assert L.cls_connect_batch(e.h, C.byref(cs), n, outs[i][j].data_ptr(),
                                       _abi.F_DEVICE | _abi.F_COUNT, s) == _abi.OK
            if i == 0:
                assert L.cls_connect_rules(e.h, C.byref(cs), n, tv[j].data_ptr(), tr_out[j].data_ptr(),
                                           _abi.F_DEVICE, s) == _abi.OK

    def hosted(i):
        for j in range(K):
            _same(e.connect_batch(*host, count=True), want, "host thread %d call %d" % (i, j))
    _run([lambda i=i: device(i) for i in range(n_dev)] + [lambda i=i: hosted(i) for i in range(2)], e)
    _sync()
    for i in range(n_dev):
        for j in range(K):
            _same(_np(outs[i][j], np.uint8), want, "device thread %d call %d" % (i, j))
    for j in range(K):
        _same(_np(tv[j], np.uint8), want, "trace call %d: verdicts" % j)
        _same(_np(tr_out[j], np.int32), rows, "trace call %d: rules" % j)
    total = 0
    for name in c["by_name"]:
        got = e.conn_counters(name, reset=True)
        tc.sums_to(got, [c["counts"][name]] * (T * K))
        total += int(got.sum())
        assert not e.conn_counters(name).any(), name
    assert total > T * K * n // 4


# ---- 5: the four reach calls at once --------------------------------------------

def _matrix_sums(v):
    hist = np.stack([np.bincount(v[p].ravel(), minlength=4)[:4] for p in range(len(v))]).astype(np.uint64)
    return hist, (v == rc.ALLOW).sum(axis=2).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def ports_ref(fam):
    """Six endpoints of the case (reach_ports_cases.brute_endpoints) at the
    class starts: (endpoints, ranges_ref's tuple, K)."""
    c = rc.case(fam)
    eps = np.array(pc.brute_endpoints(fam, 0))
    starts = pc.class_starts(pc.bound_rules(c, eps), 0)
    v = pc.oracle_at(fam, eps, 0, starts)
    return eps, pc.ranges_ref(v, starts), len(starts)


@pytest.mark.parametrize("fam", [4, 16])
def test_four_reach_calls_at_once(installed, libopt, fam):
    """cls_reach_matrix, _diff, _ports and _hops, two threads each, K device
    calls on their own streams under reach_tile=1024 (several tiles a call):
    the r_* scratch, reach_up and the connection scratch of every tile."""
    import torch
    e, _, ids = installed(fam)
    libopt.set("reach_tile", 1024, e)
    c, aft = rc.case(fam), dc.after(fam)
    want = c["want"]
    args = (ids, c["addrs"], c["pr"], c["sp"], c["dp"])
    whist, wallow = _matrix_sums(want)
    rec, total, trans, changed = dc.diff_ref(aft["want"], want)
    assert total > 0
    eps, (prec, ptotal, pruns, pallow, phist), pk = ports_ref(fam)
    assert len(eps) ** 2 * pk > 2 * 1024
    whops = hc.hops_ref(hc.adjacency(want))
    wsums = hc.sums(whops)
    base = _dev(aft["want"])
    cap = ptotal + 5
    ranges = {i: [torch.full((cap, 4), -1, dtype=torch.int32, device="cuda") for _ in range(K)] for i in (2, 6)}
    streams = _streams(T)
    res = [[] for _ in range(T)]
    _sync()

    def caller(i):
        s = streams[i]
        for j in range(K):
            kind = i % 4
            if kind == 0:
                r = e.reach_matrix(*args, out=(None, None, None), stream=s)
            elif kind == 1:
                r = e.reach_diff(*args, base, hist=True, allow=True, stream=s)
            elif kind == 2:
                r = e.reach_ports(ids[eps], c["addrs"][eps], 0, pc.SPORT[0], out=(ranges[i][j], None, None, None, None),
                                  stream=s)
            else:
                r = e.reach_hops(*args, closure=True, out=(None,) * 5, stream=s)
            res[i].append(r)
    _run([lambda i=i: caller(i) for i in range(T)], e)
    _sync()
    for i in range(T):
        assert len(res[i]) == K
        for j, r in enumerate(res[i]):
            what = "thread %d call %d" % (i, j)
            if i % 4 == 0:
                _same(_np(r[0], np.uint8), want, what + ": matrix")
                _same(_np(r[1], np.uint64), whist, what + ": hist")
                _same(_np(r[2], np.uint32), wallow, what + ": allow")
            elif i % 4 == 1:
                _same(_np(r.verdicts, np.uint8), want, what + ": diff verdicts")
                assert int(r.n_changes[0]) == total, what
                got = np.ascontiguousarray(r.changes.cpu().numpy()[:total]).view(_abi.REACH_CHANGE).reshape(-1)
                assert got.tobytes() == rec.tobytes(), what + ": records"
                _same(_np(r.trans, np.uint64), trans, what + ": trans")
                _same(_np(r.changed, np.uint32), changed, what + ": changed")
                _same(_np(r.hist, np.uint64), whist, what + ": diff hist")
                _same(_np(r.allow, np.uint32), wallow, what + ": diff allow")
            elif i % 4 == 2:
                assert r.n_classes == pk and int(r.n_ranges[0]) == ptotal, what
                got = r.ranges.cpu().numpy()
                assert got[:ptotal].tobytes() == prec.tobytes(), what + ": ranges"
                assert (got[ptotal:] == -1).all(), what + ": records past the total"
                _same(_np(r.runs, np.uint32), pruns, what + ": runs")
                _same(_np(r.allow_ports, np.uint32), pallow, what + ": allow_ports")
                _same(_np(r.hist, np.uint64), phist, what + ": ports hist")
            else:
                kinds = (np.uint8, np.uint32, np.uint32, np.uint64, np.uint64)
                for name, g, w, kd in zip(r._fields, r, (whops,) + wsums, kinds):
                    _same(_np(g, kd), w, "%s: %s" % (what, name))


# ---- 6: atomicity under ACL churn --------------------------------------------

@pytest.mark.parametrize("fam", [4, 16])
def test_acl_churn_is_atomic(fam):
    """A writer toggles one local ACL between R0 and R1 = deny-any + R0 forty
    times, ending on R1; four readers run host connection batches of the
    case's 4,107 rows and three the host reach matrix of twelve probes --
    16,428 cells -- under reach_tile=256, until it is done.  The library
    rounds the option up to 1024 connections, its smallest tile, so one locked
    matrix call is 17 tiles: counted before the threads start from the
    launches debug_conn prints.  Every result is the whole matrix of R0 or of
    R1, which differ in >= 5 % of the cells (test_thread_cases_cpu.py): never
    a mix.  No counters: a re-put starts a new table."""
    c, ch = rc.case(fam), tc.churn_case(fam)
    flat = [ch["want0"].ravel(), ch["want1"].ravel()]
    states = [ch["big0"], ch["big1"]]
    e = _engine(options={"reach_tile": 256})
    try:
        ep_ids = rc.install(e, c)
        if_ids = np.array([e.if_id(x) for x in c["ifs"]], np.uint32)
        host = _conn_host(c, if_ids)
        args = (ep_ids, c["addrs"], ch["pr"], ch["sp"], ch["dp"])
        # the tiles of one matrix call, as the library launches them
        capfd = CAPTURE[0]
        e.set_option("debug_conn", 1)
        capfd.readouterr()
        _same(e.reach_matrix(*args, hist=False, allow=False)[0], states[0], "matrix before the churn")
        launched = [int(ln.split()[2]) for ln in capfd.readouterr().err.splitlines() if ln.startswith("connect: n ")]
        e.set_option("debug_conn", None)
        assert len(launched) >= 17 and len(launched) == tc.tiles(states[0].size, 256), launched
        assert sum(launched) == states[0].size and max(launched) == tc.lib_reach_tile(256), launched
        done = threading.Event()

        def writer():
            try:
                for k in range(40):
                    assert e.acl_put(ch["name"], ch["r1"] if k & 1 else ch["r0"], ch["ing"], ch["eg"]) == 0
            finally:
                done.set()

        def conn_reader():
            seen = [0, 0]
            while not done.is_set():
                seen[tc.one_of(e.connect_batch(*host), flat)] += 1
            return seen

        def matrix_reader():
            seen = [0, 0]
            while not done.is_set():
                seen[tc.one_of(e.reach_matrix(*args, hist=False, allow=False)[0], states)] += 1
            return seen
        res = _run([writer] + [conn_reader] * 4 + [matrix_reader] * 3, e)
        print("acl churn af %d: states seen per reader %s" % (fam, res[1:]))
        _same(e.connect_batch(*host), flat[1], "connections after the last put")
        _same(e.reach_matrix(*args, hist=False, allow=False)[0], states[1], "matrix after the last put")
    finally:
        e.close()


# ---- 7: options flipped under load ---------------------------------------------

FLIPS = [("other_cap", (0, 1000)), ("fold_split", (0, 1)), ("conn_bitmap", (0, 1)), ("conn_pair", (0, 1)),
         ("conn_pair16", (0, 1)), ("conn_pre_rules", (0, 1)), ("conn_pre_narrow", (0, 1)), ("conn_jobs", (0, 1)),
         ("pair_o4", (0, 1)), ("pair_class", (0, 1)), ("reach_tile", (256, 4096, None)), ("hops_rows", (4, 8, 16))]
# (reach_tile: the library rounds up to a multiple of 1024, so 256 is 1024 connections -- the case's 4,107 cells
# in 5 tiles, then 2, then the default's one)


@pytest.mark.parametrize("fam", [4, 16])
def test_options_flipped_under_load(installed, fam):
    """One thread cycles the launch-plan switches (no compiler option, no
    debug_* one) while three classify, two run device connection batches --
    every set_option bumps conn_gen: a replan and a conn_quiesce -- and two
    run cls_reach_hops: Opts read by the launches, conn_gen, the kept plan.
    (Seven workers and the flipper: eight threads.)  Everything stays exact;
    the defaults are back afterwards."""
    L = _abi.lib()
    e, if_ids, ids = installed(fam)
    c = rc.case(fam)
    want = c["want"]
    rules, batches = classify_case(fam)
    n = want.size
    whops = hc.hops_ref(hc.adjacency(want))
    wsums = hc.sums(whops)
    t = e.put_table("flip", rules)
    try:
        devs = [_to_device(b[0]) for b in batches[:3]]
        outs = [Outs(K, N, len(rules)) for _ in range(3)]
        d = [_dev(x) for x in _conn_host(c, if_ids)]
        cs = _conn_soa(fam, d)
        couts = [_conn_outs(K, n) for _ in range(2)]
        streams = _streams(7)
        hres = [[], []]
        _sync()

        def flipper():
            for _ in range(2):
                for key, values in FLIPS:
                    for v in values:
                        e.set_option(key, v)

        def conn(i):
            for j in range(K):
                assert L.cls_connect_batch(e.h, C.byref(cs), n, couts[i][j].data_ptr(), _abi.F_DEVICE,
                                           streams[3 + i].cuda_stream) == _abi.OK

        def hops(i):
            for j in range(K):
                hres[i].append(e.reach_hops(ids, c["addrs"], c["pr"], c["sp"], c["dp"], closure=True,
                                            out=(None,) * 5, stream=streams[5 + i]))
        try:
            _run([flipper] + [lambda i=i: _classify_calls(e, t, devs[i], outs[i], streams[i]) for i in range(3)] +
                 [lambda i=i: conn(i) for i in range(2)] + [lambda i=i: hops(i) for i in range(2)], e)
        finally:
            if e.h:
                for key, _ in FLIPS:
                    e.set_option(key, None)
        _sync()
        for i in range(3):
            outs[i].check(batches[i], "classify thread %d" % i)
        for i in range(2):
            for j in range(K):
                _same(_np(couts[i][j], np.uint8), want.ravel(), "connection thread %d call %d" % (i, j))
            kinds = (np.uint8, np.uint32, np.uint32, np.uint64, np.uint64)
            for j, r in enumerate(hres[i]):
                for name, g, w, kd in zip(r._fields, r, (whops,) + wsums, kinds):
                    _same(_np(g, kd), w, "hops thread %d call %d: %s" % (i, j, name))
    finally:
        if e.h:
            e.del_table(t)


# ---- 8: a multi-device engine on one GPU ----------------------------------------

@pytest.mark.parametrize("af", [4, 16])
def test_multi_device_engine_on_one_gpu(af):
    """devices = [0, 0, 0], no communicator.  Two threads loop upload ->
    cls_classify_batch -> cls_batch_counters -> download on batches of their
    own, one classifies through the peer handle of device 2, one puts and
    deletes tables on the primary (sync_peers takes every peer's lock), one
    runs cls_batch_connect + cls_batch_wait and reads cls_conn_counters with
    reset after each (only this thread counts, so every read is the oracle's
    counts once): the pinned stage[2], the peers' locks (primary first, then
    device order) of the table sync and of the counter merge, the peers'
    mirrored tables.  A lock-order mistake shows as the deadline."""
    from batch_cases import INPUTS, two_tables
    from test_gpu_batches import _install, _upload
    from vpp_amd.engine import Table
    k = K
    small, big, tr, (sv, sc), (bv, bc) = two_tables(af)
    n = len(tr["dport"])
    e = _engine(devices=[0, 0, 0])
    try:
        assert e.n_devices() == 3 and e.comm_info() == (0, 0)
        case, cb = _install(e, af)
        ts, tb = e.put_table("small", small), e.put_table("big", big)
        peer = e.device_engine(2)
        tp = Table(peer, tb.id, tb.n_rules, "big")
        mine = [e.batch(n, af=af) for _ in range(2)]
        for name in case["by_name"]:
            e.conn_counters(name, reset=True)

        def batches(i):
            b, t, wv, wc = mine[i], (ts, tb)[i], (sv, bv)[i], (sc, bc)[i]
            for j in range(k):
                b.upload(_abi.BF_VERDICT, np.full(n, 0xEE, np.uint8))
                _upload(b, tr, INPUTS)
                _same(e.classify_batch(t, b), wc, "batch %d call %d: merged counters" % (i, j))
                _same(b.counters(t.n_rules), wc, "batch %d call %d: cls_batch_counters" % (i, j))
                _same(b.download(_abi.BF_VERDICT), wv, "batch %d call %d: verdicts" % (i, j))

        def through_peer():
            for j in range(k):
                v, c_ = peer.classify(tp, tr["src"], tr["dst"], tr["dport"], tr["proto"])
                _same(v, bv, "peer call %d: verdicts" % j)
                _same(c_, bc, "peer call %d: counters" % j)

        def tables():
            for j in range(2 * k):
                t = e.put_table("churn%d" % j, small)
                assert t.info()["n_rules"] == len(small)
                e.del_table(t)

        def connections():
            for j in range(k):
                cb.upload(_abi.BF_VERDICT, np.full(case["n"], 0xEE, np.uint8))
                e.connect_batch_b(cb, mode="classifier", count=True)
                cb.wait()
                _same(cb.download(_abi.BF_VERDICT), case["want"], "connections call %d" % j)
                for name in case["by_name"]:
                    _same(e.conn_counters(name, reset=True), case["counts"][name], "call %d: %s" % (j, name))
        _run([lambda: batches(0), lambda: batches(1), through_peer, tables, connections], e)
        for name in case["by_name"]:
            assert not e.conn_counters(name).any(), name
    finally:
        e.close()


# ---- 9: two engines on one device -------------------------------------------------

@pytest.mark.parametrize("af", [4, 16])
def test_two_engines_one_device(af):
    """A thread per engine: scenario 1's calls on its own stream and a table
    put and delete between them.  Nothing is shared but the process: the
    kernels' one-time attributes (lds_attr) and once-flags, the compiler."""
    rules, batches = classify_case(af)
    small = random_acl(801, 40, 0.05)[0]
    engs = [_engine(), _engine()]
    try:
        ts = [e.put_table("mine", rules) for e in engs]
        devs = [_to_device(batches[i][0]) for i in range(2)]
        outs = [Outs(K, N, len(rules)) for _ in range(2)]
        streams = _streams(2)
        _sync()

        def caller(i):
            def put(j):
                engs[i].del_table(engs[i].put_table("t%d" % j, small))
            _classify_calls(engs[i], ts[i], devs[i], outs[i], streams[i], each=put)
        _run([lambda i=i: caller(i) for i in range(2)], *engs)
        _sync()
        for i in range(2):
            outs[i].check(batches[i], "engine %d" % i)
    finally:
        for e in engs:
            e.close()


# ---- 10: the generators -----------------------------------------------------------

@pytest.mark.parametrize("af", [4, 16])
def test_generators(eng, af):
    """cls_gen_traffic_v4 / _v16 from eight threads with different specs and
    first packets into their own arrays on their own streams: the shared pool
    upload (s_pool, gen_pairs, gen_pending)."""
    import torch
    from vpp_amd import workload
    k = K
    spec0 = workload.config(5 if af == 16 else 2)[1]
    gen = oracle.gen_traffic_v16 if af == 16 else oracle.gen_traffic_v4
    shape = (N, 16) if af == 16 else (N,)
    adt = torch.uint8 if af == 16 else torch.int32
    specs = [dict(spec0, seed=1234 + i, pct_pod_src=30 + 5 * i, pct_icmp=i) for i in range(T)]
    firsts = [[1000003 * i + 77 * j for j in range(k)] for i in range(T)]
    want = [[gen(specs[i], firsts[i][j], N) for j in range(k)] for i in range(T)]
    outs = [[{"src": torch.empty(shape, dtype=adt, device="cuda"), "dst": torch.empty(shape, dtype=adt, device="cuda"),
              "sport": torch.empty(N, dtype=torch.int16, device="cuda"),
              "dport": torch.empty(N, dtype=torch.int16, device="cuda"),
              "proto": torch.empty(N, dtype=torch.uint8, device="cuda")} for _ in range(k)] for _ in range(T)]
    streams = _streams(T)
    fn = eng.gen_traffic_v16 if af == 16 else eng.gen_traffic_v4
    _sync()

    def caller(i):
        for j in range(k):
            fn(specs[i], firsts[i][j], outs[i][j], stream=streams[i])
    _run([lambda i=i: caller(i) for i in range(T)], eng)
    _sync()
    assert not np.array_equal(want[0][0]["src"], want[1][0]["src"])
    for i in range(T):
        for j in range(k):
            for f, w in want[i][j].items():
                _same(_np(outs[i][j][f], w.dtype), w, "thread %d call %d: %s" % (i, j, f))


# ---- the options no other test sets (one thread) ---------------------------------

N_WIDE = 300007          # more than 64 workgroups


@functools.lru_cache(maxsize=None)
def wide_case(af):
    rules, b = classify_case(af, N_WIDE, 1)
    tr, ov, _, oc = b[0]
    return rules, tr, ov, oc


@pytest.mark.parametrize("wg", [1, 2])
@pytest.mark.parametrize("fold_split", [0, 1])
@pytest.mark.parametrize("af", [4, 16])
def test_fold_split_and_wg_per_cu(eng, libopt, af, fold_split, wg):
    """The finish launch with a slot tile's rows over several blocks or one
    block per tile, one or two classify workgroups per CU.  finish_args takes
    split > 1 when the slot tiles -- 64 slots each, of the main image's slots,
    the OTHER image's and one per rule and the default DENY -- are at most
    half the CUs.  The slot counts are the compiler's for these rules under
    its defaults (the options set here are launch-plan ones); for IPv4 the
    engine's table reports the main image's count, which must agree.  The
    16-byte table reports none, so its count is the compiler's alone."""
    import torch
    from cls_image import Image, Image16, compile_blob
    rules, tr, ov, oc = wide_case(af)
    cr = _abi.CRules(rules)
    main = Image16(compile_blob(cr, "cls_compile_v16")).core if af == 16 else Image(compile_blob(cr))
    assert main.other is not None
    slots = main.h.n_ctr + main.other.h.n_ctr + len(rules) + 1
    libopt.set("fold_split", fold_split, eng)
    libopt.set("wg_per_cu", wg, eng)
    t = eng.put_table("wide", rules)
    try:
        info = t.info()
        cu = torch.cuda.get_device_properties(0).multi_processor_count
        assert info["lds_resident_v16" if af == 16 else "lds_resident"] == 1
        if af == 4:
            assert info["n_slots"] == main.h.n_ctr
        assert (slots + 63) // 64 <= cu // 2, (slots, cu)
        v, c = eng.classify(t, tr["src"], tr["dst"], tr["dport"], tr["proto"])
        d = _to_device(tr)
        dv = torch.full((N_WIDE,), 0xEE, dtype=torch.uint8, device="cuda")
        dc_ = torch.zeros(len(rules) + 1, dtype=torch.int64, device="cuda")
        _sync()
        eng.classify(t, d["src"], d["dst"], d["dport"], d["proto"], verdict=dv, counters=dc_)
        _sync()
    finally:
        eng.del_table(t)
    _same(v, ov, "host verdicts")
    _same(c, oc, "host counters")
    _same(_np(dv, np.uint8), ov, "device verdicts")
    _same(_np(dc_, np.uint64), oc, "device counters")


@pytest.mark.parametrize("wg", [1, 2])
@pytest.mark.parametrize("fam", [4, 16])
def test_conn_wg_per_cu(installed, libopt, fam, wg):
    """The connection kernel capped at one or two workgroups per CU: counted
    classifier-mode and automatic batches of the case."""
    e, if_ids, _ = installed(fam)
    c = rc.case(fam)
    libopt.set("conn_wg_per_cu", wg, e)
    host = _conn_host(c, if_ids)
    for name in c["by_name"]:
        e.conn_counters(name, reset=True)
    for mode in ("classifier", "auto"):
        _same(e.connect_batch(*host, mode=mode, count=True), c["want"].ravel(), mode)
        got = e.connect_batch(*[_dev(x) for x in host], mode=mode, count=True)
        _sync()
        _same(_np(got, np.uint8), c["want"].ravel(), mode + ", device")
    for name in c["by_name"]:
        tc.sums_to(e.conn_counters(name, reset=True), [c["counts"][name]] * 4)


def test_phash_sparse(eng, libopt):
    """phash_dense=0 (at least two port-hash slots per port) on the
    rendered-table shape, whose list mode hashes the port classes."""
    rules, pool = single_port_acl(7, 300, n_prefixes=3)
    tr = random_traffic(9, N, pool)
    ov, oc = oracle.classify_fast(oracle.rules_to_c(rules), tr["src"], tr["dst"], tr["dport"], tr["proto"])
    libopt.set("phash_dense", 0, eng)
    t = eng.put_table("sparse", rules)
    try:
        assert t.info()["list_mode"] == 4
        v, c = eng.classify(t, tr["src"], tr["dst"], tr["dport"], tr["proto"])
    finally:
        eng.del_table(t)
    _same(v, ov, "verdicts")
    _same(c, oc, "counters")


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_batch_layouts(libopt, layout):
    """The three placements of a batch's field arrays (packed, one allocation
    per field, staggered) on batch_cases.case16 over two shards."""
    from batch_cases import INPUTS, case16
    from test_gpu_batches import _upload
    rules, tr, ov, oc = case16()
    e = _engine(devices=[0, 0])
    try:
        libopt.set("batch_layout", layout, e)
        t = e.put_table("t", rules)
        b = e.batch(len(ov), af=_abi.AF_V16)
        b.upload(_abi.BF_VERDICT, np.full(len(ov), 0xEE, np.uint8))
        _upload(b, tr, INPUTS)
        _same(e.classify_batch(t, b), oc, "counters")
        _same(b.download(_abi.BF_VERDICT), ov, "verdicts")
    finally:
        e.close()
