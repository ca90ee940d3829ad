"""GPU: every classify variant in its full-step loop and at every depth.

classify4_cls (vpp_amd/csrc/kernels_dev.hpp) runs its full-grid-step loop --
the only one with the depth-specialised search, the ordered loads and the
cached protocol load -- only when the batch holds at least one step for every
thread of the grid; below the saturated grid that means a multiple of 4096
packets (tests/classify_steps_cases.py, pinned on the CPU by
tests/test_classify_steps_cpu.py).  The other parity tests send batches that
stay in the leftover loop and the per-packet tail.  Here every test first
asserts, from the device's CU count and the table's own info, which loops its
batch reaches, then compares bit for bit: verdicts and per-rule counters
against the evalACL oracle (oracle.classify_fast), verdicts also against the
linear kernel (force_linear), matched rules against the oracle's trace.
"""
import numpy as np
import pytest

import classify_steps_cases as K
import oracle
from aclgen import directed_traffic, random_acl, random_traffic, single_port_acl
from cls_image import Image, Image16, compile_blob
from vpp_amd import _abi

pytestmark = pytest.mark.gpu

OTHER_SEGS = 16       # kOtherSegs: OTHER queue segments (waves) per workgroup


@pytest.fixture(scope="module")
def eng():
    from vpp_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same(got, want, what=""):
    v, c = got
    ov, oc = want
    bad = np.nonzero(v != ov)[0]
    assert len(bad) == 0, "%s verdict mismatch at %s: got %s want %s" % (what, bad[:8], v[bad[:8]], ov[bad[:8]])
    np.testing.assert_array_equal(c, oc, err_msg=what)


def _oracle(rules, tr, af=4):
    return oracle.classify_fast(oracle.rules_to_c(rules), tr["src"], tr["dst"], tr["dport"], tr["proto"], af=af)


def _classify(eng, t, tr, want):
    _same(eng.classify(t, tr["src"], tr["dst"], tr["dport"], tr["proto"]), want, "classifier")
    v, _ = eng.classify(t, tr["src"], tr["dst"], tr["dport"], tr["proto"], force_linear=True)
    assert np.array_equal(v, want[0]), "linear kernel"


def _header(rules, fn="cls_compile_v4", **extra):
    """The header of the image the engine compiles under the test's options."""
    blob = compile_blob(_abi.CRules(rules), fn, options={k: str(v) for k, v in extra.items()})
    return Image16(blob).h if fn == "cls_compile_v16" else Image(blob).h


def _saturated_n(n_cu, info, rounds=1):
    """The batch of `rounds` full rounds, 777 leftover groups and a 3-packet
    tail on this table and device, its census asserted."""
    lds = info["lds_resident"] == 1
    n = K.saturated(n_cu, K.per_cu(lds), rounds, 777, 3)
    assert K.census4(n, n_cu, lds) == (n_cu * K.per_cu(lds), rounds, 777, 3)
    return n


# ---------------------------------------------------------------------------
# 1. every (source lookup, list mode) variant on both sides of the path change

def _variant_table(kind, libopt, eng):
    from test_gpu_parity import VARIANTS, variant_acl
    libopt.set("orient", "src", eng)
    if kind.endswith("_pc"):
        libopt.set("list_mode_max", "2", eng)
    libopt.set("trie", "1" if kind.startswith("trie") else "0", eng)
    libopt.set("src_search", "1" if kind.startswith(("search", "trie")) else "0", eng)
    rules, pool = variant_acl(kind, 0)
    h = _header(rules)
    assert (h.mode, h.list_mode) == VARIANTS[kind], kind
    return rules, pool


KINDS = ["hash_bv", "hash_cbv", "hash_pc", "hash_scan", "hash_sph", "host_cbv", "host_sph", "hrow_cbv", "hrow_sph",
         "search_bv", "search_cbv", "search_pc", "search_scan", "search_sph", "trie_cbv", "trie_sph"]


def test_kinds_are_all_the_variants():
    from test_gpu_parity import VARIANTS
    assert KINDS == sorted(VARIANTS)


@pytest.mark.parametrize("kind", KINDS)
def test_every_variant_in_the_full_step_loop(eng, n_cu, libopt, kind):
    """One round with every packet in the full-step loop, and 23 packets more
    on the same table, which has none in it (leftover loop and tail)."""
    rules, pool = _variant_table(kind, libopt, eng)
    t = eng.put_table("v", rules)
    try:
        lds = t.info()["lds_resident"] == 1
        for n, census in ((K.one_round(3), (3, 1, 0, 0)), (K.one_round(3) + 4 * 5 + 3, (4, 0, 3 * 1024 + 5, 3))):
            assert K.census4(n, n_cu, lds) == census
            tr = directed_traffic(rules, random_traffic(11, n, pool), 0, share=0.5)
            _classify(eng, t, tr, _oracle(rules, tr))
    finally:
        eng.del_table(t)


# ---------------------------------------------------------------------------
# 2. every depth: kD = 0 .. 5 and the run-time fallback (6, 7)

@pytest.mark.parametrize("depth,lookup,list_mode", K.DEPTH_CASES)
def test_every_depth_in_the_full_step_loop(eng, n_cu, libopt, depth, lookup, list_mode):
    c = K.for_depth(depth, lookup, list_mode)
    c.apply(libopt, eng)
    h = _header(c.rules)
    assert (h.mode, h.list_mode, h.bv_steps_d, h.bv_steps_p) == (c.mode, list_mode, depth, 0)
    assert (h.n_hash == 1) == (lookup == "host")
    t = eng.put_table("d", c.rules)
    try:
        info = t.info()
        # the depth-specialised launch: LDS-resident image, u32 LDS counters
        assert (info["kernel"], info["lds_resident"], info["ctr16"], info["list_mode"]) == (1, 1, 0, list_mode)
        n = K.one_round(2)
        assert K.census4(n, n_cu, True) == (2, 1, 0, 0)
        tr = K.ladder_traffic(c, n, other_every=16)
        assert K.reached(c, tr, n)
        _classify(eng, t, tr, _oracle(c.rules, tr))
    finally:
        eng.del_table(t)


# ---------------------------------------------------------------------------
# 3. one launch through all three loops

@pytest.mark.parametrize("key", sorted(K.SATURATED))
def test_one_launch_through_all_three_loops(eng, n_cu, libopt, key):
    c = K.saturated_case(key)
    c.apply(libopt, eng)
    t = eng.put_table("s", c.rules)
    try:
        info = t.info()
        assert info["lds_resident"] == 1 and info["ctr16"] == 0
        n = _saturated_n(n_cu, info)
        tr = K.ladder_traffic(c, n, other_every=16)
        assert K.reached(c, tr, 4 * n_cu * K.BLOCK)
        _classify(eng, t, tr, _oracle(c.rules, tr))
    finally:
        eng.del_table(t)


@pytest.mark.parametrize("key", ["ladder9", "search", "host"])
def test_all_three_loops_on_a_global_image(eng, n_cu, libopt, key):
    """No image of the table fits the LDS budget: two workgroups per CU, so a
    saturated batch of about 2 Mi packets (the source trie exists only in
    LDS-resident images)."""
    c = K.saturated_case(key)
    c.apply(libopt, eng)
    libopt.set("lds_budget", "256", eng)
    libopt.set("list_mode", "4", eng)
    h = _header(c.rules)
    assert (h.mode, h.n_hash == 1, h.list_mode) == (c.mode, key == "host", 4)
    t = eng.put_table("g", c.rules)
    try:
        info = t.info()
        assert info["lds_resident"] == 0 and info["kernel"] == 1
        n = _saturated_n(n_cu, info)
        assert n > 2 * n_cu * 4096
        tr = K.ladder_traffic(c, n, other_every=16)
        assert K.reached(c, tr, 8 * n_cu * K.BLOCK)
        _classify(eng, t, tr, _oracle(c.rules, tr))
    finally:
        eng.del_table(t)


def test_two_rounds_on_the_config2_table_device_arrays(eng, n_cu):
    """Two full rounds, leftovers and a tail over device-generated traffic in
    device arrays; the oracle over the whole batch."""
    import torch
    from vpp_amd import workload
    acl, spec, _ = workload.config(2)
    t = eng.put_table("cfg2", acl.rules)
    try:
        info = t.info()
        assert info["kernel"] == 1 and info["lds_resident"] == 1
        n = _saturated_n(n_cu, info, rounds=2)
        out = {k: torch.empty(n, dtype=dt, device="cuda") for k, dt in
               (("src", torch.int32), ("dst", torch.int32), ("sport", torch.int16), ("dport", torch.int16),
                ("proto", torch.uint8))}
        eng.gen_traffic_v4(spec, 0, out)
        verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
        counters = torch.zeros(t.n_rules + 1, dtype=torch.int64, device="cuda")
        eng.classify(t, out["src"], out["dst"], out["dport"], out["proto"], verdict=verdict, counters=counters)
        vl = torch.empty(n, dtype=torch.uint8, device="cuda")
        eng.classify(t, out["src"], out["dst"], out["dport"], out["proto"], verdict=vl, force_linear=True)
        torch.cuda.synchronize()
        tr = oracle.gen_traffic_v4(spec, 0, n)
        want = _oracle(acl.rules, tr)
        _same((verdict.cpu().numpy(), counters.cpu().numpy().astype(np.uint64)), want, "classifier")
        assert np.array_equal(vl.cpu().numpy(), want[0]), "linear kernel"
    finally:
        eng.del_table(t)


# ---------------------------------------------------------------------------
# 4. counter tiers and wide cells

def _tier_table(eng, libopt, rules, tier):
    """The table put in counter tier `tier` (test_gpu_counters._check's
    recipe: the budget sized on the layout, the layout then held)."""
    from test_gpu_counters import _budget
    libopt.set("orient", "src", eng)
    h = _header(rules)
    assert h.has_cls
    libopt.set("lds_budget", str(_budget(h, tier)), eng)
    libopt.set("list_mode", str(h.list_mode), eng)
    libopt.set("trie", "1" if h.mode == 4 else "0", eng)
    t = eng.put_table("tier", rules)
    info = t.info()
    if tier == "global":
        assert info["lds_resident"] == 0
    else:
        assert info["lds_resident"] == 1 and info["ctr16"] == (0 if tier == "u32" else 1)
        assert (info["n_lctr"] < info["n_slots"]) == (tier == "partial")
    return t, info, h.list_mode


@pytest.mark.parametrize("tier", ["u32", "u16", "partial", "global"])
@pytest.mark.parametrize("seed,weird,list_mode", [(0, 0.05, 4), (1, 0.0, 3)])
def test_counter_tiers_in_the_full_step_loop(eng, n_cu, libopt, seed, weird, list_mode, tier):
    rules, pool = random_acl(seed * 101 + 17, 400, weird)
    t, info, lm = _tier_table(eng, libopt, rules, tier)
    try:
        assert lm == list_mode
        n = K.one_round(3)
        assert K.census4(n, n_cu, info["lds_resident"] == 1) == (3, 1, 0, 0)
        for n in (n, _saturated_n(n_cu, info)):
            tr = random_traffic(seed + 3, n, pool)
            _classify(eng, t, tr, _oracle(rules, tr))
    finally:
        eng.del_table(t)


@pytest.mark.parametrize("list_mode", [5, 6])
@pytest.mark.parametrize("lookup", ["search", "hash", "host", "trie"])
def test_wide_cells_in_the_full_step_loop(eng, n_cu, libopt, list_mode, lookup):
    """Wide cells (list mode 5: the wide form of 4, 6: of 3) under every
    source lookup: the interval search and the trie over a 200-rule table of
    60 prefixes, the hashes over the depth-4 ladder."""
    if lookup in ("hash", "host"):
        c = K.for_depth(4, lookup, 4)
        c.apply(libopt, eng)
        rules = c.rules
        gen = lambda n: K.ladder_traffic(c, n, other_every=16)
    else:
        libopt.set("orient", "src", eng)
        libopt.set("trie", "1" if lookup == "trie" else "0", eng)
        rules, pool = single_port_acl(5, 200, n_prefixes=60)
        gen = lambda n: random_traffic(2, n, pool)
    libopt.set("wide", "1", eng)
    if list_mode == 6:
        libopt.set("list_mode_max", "3", eng)
    h = _header(rules)
    assert (h.mode, h.n_hash == 1, h.list_mode) == (K.LOOKUPS[lookup][1], lookup == "host", list_mode)
    t = eng.put_table("w", rules)
    try:
        info = t.info()
        assert info["list_mode"] == list_mode and info["lds_resident"] == 1
        n = K.one_round(3)
        assert K.census4(n, n_cu, True) == (3, 1, 0, 0)
        for n in (n, _saturated_n(n_cu, info)):
            tr = gen(n)
            _classify(eng, t, tr, _oracle(rules, tr))
    finally:
        eng.del_table(t)


# ---------------------------------------------------------------------------
# 5. the OTHER queue across the loops

def _queue_demand(proto, grid, rounds):
    """Queue entries each wave asks for, per loop: one per lane whose group of
    four holds a protocol > 2 (full rounds, leftover groups), one per tail
    packet.  Returns (per round [waves], leftover [waves], tail [waves])."""
    n = len(proto)
    nthreads = grid * K.BLOCK
    waves = nthreads // 64
    nsteps = n // 4
    assert nsteps // nthreads == rounds
    lanes = (proto[:4 * nsteps] > 2).reshape(-1, 4).any(1)
    per_round = [lanes[k * nthreads:(k + 1) * nthreads].reshape(waves, 64).sum(1) for k in range(rounds)]
    left = np.zeros(nthreads, np.int64)
    left[:nsteps - rounds * nthreads] = lanes[rounds * nthreads:]
    tail = np.zeros(nthreads, np.int64)
    tail[:n - 4 * nsteps] = proto[4 * nsteps:] > 2
    return per_round, left.reshape(waves, 64).sum(1), tail.reshape(waves, 64).sum(1)


@pytest.mark.parametrize("cap,rounds", [(256, 2), (None, 2), (None, 1)])
def test_other_queue_across_the_loops(eng, n_cu, libopt, cap, rounds):
    """Full rounds, leftovers and a tail with every tenth packet of protocol
    47 (and one of the tail's).  cap 256: 16 entries per wave, fewer than any
    wave asks for in round 1, so every segment fills there and the second
    round, the leftover loop and the tail classify in place.  The default
    cap (engine.cpp other_cap) over two rounds: both rounds are queued whole,
    the first waves fill in the leftover loop.  Over one round: everything is
    queued, and the finish launch drains the masks written by the groups of
    four and by the tail's single packets."""
    c = K.saturated_case("ladder9")
    c.apply(libopt, eng)
    if cap is not None:
        libopt.set("other_cap", str(cap), eng)
    t = eng.put_table("o", c.rules)
    try:
        info = t.info()
        assert info["lds_resident"] == 1
        n = _saturated_n(n_cu, info, rounds=rounds)
        tr = K.ladder_traffic(c, n, other_every=10)
        tr["proto"][n - 2] = 47
        per_round, left, tail = _queue_demand(tr["proto"], n_cu, rounds)
        assert all(22 <= r.min() and r.max() <= 28 for r in per_round)      # 256 / 10 per wave and round
        assert left[0] >= 22 and tail[0] >= 1
        seg = (cap if cap is not None else min(16384, max(1024, (n // n_cu + 15) // 16))) // OTHER_SEGS
        if cap is not None:
            assert seg < per_round[0].min()
        elif rounds == 2:
            assert sum(per_round).max() <= seg < (sum(per_round) + left)[0]
        else:
            assert (per_round[0] + left + tail).max() <= seg
        _classify(eng, t, tr, _oracle(c.rules, tr))
    finally:
        eng.del_table(t)


# ---------------------------------------------------------------------------
# 6. slot mode (cls_classify_rules): a uint4 of result words per group

def _device(tr, shift=0):
    """The batch in torch device tensors; shift 1: each sliced by one element
    of a larger allocation, so no array is 16-byte aligned (scalar kernel)."""
    import torch
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}
    out = {}
    for k in ("src", "dst", "dport", "proto"):
        v = np.ascontiguousarray(tr[k])
        v = v.view(signed.get(v.dtype, v.dtype))
        if shift:
            v = np.concatenate([v[:shift], v])
        out[k] = torch.from_numpy(v).cuda()[shift:]
    return out


def _slots(eng, t, rules, tr, want, shift):
    import torch
    n = len(tr["dport"])
    d = _device(tr, shift)
    pad = 64
    rb = torch.full((n + pad + shift,), -1, dtype=torch.int32, device="cuda")[shift:]
    vb = torch.full((n + pad + shift,), 0xFF, dtype=torch.uint8, device="cuda")[shift:]
    rb[:n] = 3
    eng.classify_rules(t, d["src"], d["dst"], d["dport"], d["proto"], verdict=vb, rules=rb)
    torch.cuda.synchronize()
    r, v = rb.cpu().numpy().view(np.uint32), vb.cpu().numpy()
    assert (r[n:] == 0xFFFFFFFF).all() and (v[n:] == 0xFF).all(), "written past the batch"
    ov, oh = want
    bad = np.nonzero((v[:n] != ov) | (r[:n] != oh))[0]
    assert len(bad) == 0, "shift %d mismatch at %s: got %s / %s want %s / %s" % (
        shift, bad[:6], v[bad[:6]], r[bad[:6]], ov[bad[:6]], oh[bad[:6]])


SLOT_TABLES = ["hash", "search", "host", "trie", "wide"]


@pytest.mark.parametrize("key", SLOT_TABLES)
def test_slot_mode_in_the_full_step_loop(eng, n_cu, libopt, key):
    """hash, search, host: aligned arrays take the vector slot kernel (its
    three loops as the census says, a uint4 of words per group), arrays sliced
    by one element the scalar kernel (one word per packet).  trie, wide:
    dispatch_slots4 has only the scalar slot kernel for the source trie and
    for wide cells, whatever the alignment, so both calls run its per-packet
    loop alone and the census says nothing about them; they are here for the
    sizes and the outputs' bounds."""
    if key == "wide":
        libopt.set("orient", "src", eng)
        libopt.set("wide", "1", eng)
        rules, pool = single_port_acl(5, 200, n_prefixes=60)
        gen = lambda n: random_traffic(2, n, pool)
    else:
        c = K.for_depth(4, key, 4)
        c.apply(libopt, eng)
        rules = c.rules
        gen = lambda n: K.ladder_traffic(c, n, other_every=16)
    t = eng.put_table("r", rules)
    try:
        info = t.info()
        assert info["lds_resident"] == 1 and (key != "wide" or info["list_mode"] == 5)
        n1 = K.one_round(3)
        assert K.census4(n1, n_cu, True) == (3, 1, 0, 0)
        assert K.census4(n1 + 23, n_cu, True) == (4, 0, 3 * 1024 + 5, 3)
        cr = oracle.rules_to_c(rules)
        for n in (n1, n1 + 23, _saturated_n(n_cu, info)):
            tr = gen(n)
            want = oracle.classify_hits(cr, tr["src"], tr["dst"], tr["dport"], tr["proto"])
            if key != "wide" and n != n1 + 23:
                full = n if n == n1 else 4 * n_cu * K.BLOCK
                assert set(K.target_rules(c)) <= set(want[1][:full].tolist())
            _slots(eng, t, rules, tr, want, 0)              # aligned: the vector kernel (hash, search, host)
            _slots(eng, t, rules, tr, want, 1)              # sliced by one element: the scalar kernel
    finally:
        eng.del_table(t)


# ---------------------------------------------------------------------------
# 7. the 16-byte layout: its step loop always takes the template depth

N16 = 256 * 23 + 119


@pytest.mark.parametrize("key", sorted(K.TWINS))
@pytest.mark.parametrize("fe,lookup,opts", [(0, "hash", {"v16_src_search": 1}), (1, "host", {}),
                                            (2, "hash", {"v16_src_trie": 1})])
def test_16_byte_layout_at_every_depth(eng, n_cu, libopt, key, fe, lookup, opts):
    """Front ends 0 (interval search) and 1 (host-route hashes) are
    specialised on the depth, 2 (the source trie) takes it at run time."""
    libopt.set("orient", "src", eng)
    for k, v in opts.items():
        libopt.set(k, str(v), eng)
    c, rules, tr, depth = K.twin(key, lookup, N16, other_every=16)
    h = _header(rules, "cls_compile_v16")
    assert h.core.has_cls and (h.core.list_mode, h.core.bv_steps_d, h.src_mode) == (4, depth, fe)
    assert h.core.ctr16 == 0                   # u32 LDS counters: launch16_cls takes the depth branch
    assert K.census16(N16, n_cu, True) == (2, 23, 119)
    t = eng.put_table("t16", rules)
    try:
        info = t.info()
        assert info["has_v16"] == 1 and info["lds_resident_v16"] == 1
        cr = oracle.rules_to_c(rules)
        want = oracle.classify_fast(cr, tr["src"], tr["dst"], tr["dport"], tr["proto"], af=16)
        hits = oracle.classify_hits(cr, tr["src"], tr["dst"], tr["dport"], tr["proto"], af=16)
        assert set(K.target_rules(c)) <= set(hits[1][:256 * 23].tolist())
        _classify(eng, t, tr, want)
        v, r = eng.classify_rules(t, tr["src"], tr["dst"], tr["dport"], tr["proto"])
        assert np.array_equal(v, hits[0]) and np.array_equal(r, hits[1])
    finally:
        eng.del_table(t)


# ---------------------------------------------------------------------------
# 8. pair launches of connection batches

N_CONN = 4099


def _connections(rules, tr, fam, seed=3):
    """Interfaces a0..a2 under the large ACL (ingress a0, a1; egress a1, a2),
    b0 / b1 under a small one; every connection's source on a0 or a1, so the
    first evalACL call of each runs on the large ACL with the batch's tuple."""
    small, _ = random_acl(77, 5, 0.0)
    ifs = ["a0", "a1", "a2", "b0", "b1"]
    bind = {"a0": ["L", None], "a1": ["L", "L"], "a2": [None, "L"], "b0": ["S", None], "b1": [None, "S"]}
    by_name = {"L": rules, "S": small}
    acls = [("L", rules, ["a0", "a1"], ["a1", "a2"]), ("S", small, ["b0"], ["b1"])]
    rng = np.random.default_rng(seed)
    n = len(tr["dport"])
    tr = dict(tr, sport=rng.integers(1024, 65536, n).astype(np.uint16))
    si = rng.integers(0, 2, n)
    di = rng.integers(0, len(ifs), n)
    from test_gpu_connect_scale import oracle_connections
    want = oracle_connections(bind, by_name, ifs, si, di, tr, fam)
    return acls, ifs, si, di, tr, want


def _pair_run(opts, acls, ifs, si, di, tr, want, count, capfd, tag):
    from vpp_amd.engine import Engine
    eng = Engine(options=dict(opts, debug_conn=1))
    try:
        for name, rules, ing, eg in acls:
            assert eng.acl_put(name, rules, ing, eg) == 0
        ids = np.array([eng.if_id(x) for x in ifs], np.uint32)
        capfd.readouterr()
        got = eng.connect_batch(ids[si], ids[di], tr["src"], tr["dst"], tr["proto"], tr["sport"], tr["dport"],
                                mode="classifier", count=count)
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith(tag)]
        assert lines, "no pair launch"
        bad = np.nonzero(got != want[0])[0]
        assert bad.size == 0, (bad[:10], got[bad[:10]], want[0][bad[:10]])
        if count:
            for name in ("L", "S"):
                np.testing.assert_array_equal(eng.conn_counters(name, reset=True), want[1][name], err_msg=name)
    finally:
        eng.close()


PAIR4_CASES = [(d, "host", lm) for lm in (4, 3) for d in K.DEPTHS] + [(0, "hash", 4), (5, "hash", 4)]


@pytest.mark.parametrize("depth,lookup,list_mode", PAIR4_CASES)
def test_pair_launch_ipv4_at_every_depth(depth, lookup, list_mode, capfd):
    """launch_pair (k4_pair.hip) specialises classify4_pair on the depth only
    for the one-length hash (kMode 2) in list modes 3 and 4: the host ladders
    (/32 sources) at every depth, kD 0..5 and -1 for 6 and 7.  The hash
    ladders (two hashed lengths, kMode 1) take the depth at run time."""
    c = K.for_depth(depth, lookup, list_mode)
    hp = _header(c.rules, pair4=1, **c.options)
    assert (hp.mode, hp.n_hash == 1, hp.list_mode, hp.bv_steps_d, hp.bv_steps_p) == \
        (1, lookup == "host", list_mode, depth, 0)
    tr = K.ladder_traffic(c, N_CONN, other_every=16)
    acls, ifs, si, di, tr, want = _connections(c.rules, tr, 4)
    assert (want[1]["L"][K.target_rules(c)] > 0).all()        # every rung's rule and the default DENY decide a call
    assert len(set(want[0].tolist())) >= 3
    for count in (False, True):
        _pair_run(c.options, acls, ifs, si, di, tr, want, count, capfd, "pair:")


@pytest.mark.parametrize("key", sorted(K.TWINS))
def test_pair_launch_16_byte_at_every_depth(key, capfd):
    opts = {"orient": "src", "v16_src_search": 1, "conn_pair16": 1}
    c, rules, tr, depth = K.twin(key, "hash", N_CONN, other_every=16)
    hp = _header(rules, "cls_compile_v16", pair4=1, orient="src", v16_src_search=1)
    assert (hp.core.list_mode, hp.core.bv_steps_d) == (4, depth)
    acls, ifs, si, di, tr, want = _connections(rules, tr, 16)
    assert (want[1]["L"][K.target_rules(c)] > 0).all()
    for count in (False, True):
        _pair_run(opts, acls, ifs, si, di, tr, want, count, capfd, "pair16: pimg")
