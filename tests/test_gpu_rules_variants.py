"""GPU parity of the matched-rule trace (cls_classify_rules) on every
classifier variant.

The trace runs the classifier in slot mode, which has launch tables of its
own (kernels_dev.hpp dispatch_slots4 / dispatch_slots16: source lookup x list
mode, LDS-resident or global image, vector body or one packet per lane) and a
second kernel that maps each slot to its rule.  test_gpu_rules.py reaches
whatever the compiler picks for random ACLs; here the options of the classify
matrices (test_gpu_parity.py, test_gpu_v16.py, test_gpu_trie_wide.py,
test_gpu_counters.py) pin each variant, and the batches are aimed at the
rules (aclgen.directed_traffic; test_directed_traffic_cpu.py states on the
oracle what they reach).

Bar (test_gpu_rules._check): verdict and rule equal the oracle's first-match
loop element by element, and the rules' histogram equals cls_classify's
counters on the same table and batch.
"""
import numpy as np
import pytest

import oracle
from aclgen import (directed_traffic, mix_families, random_acl, random_acl16, random_traffic, random_traffic16,
                    single_port_acl)
from cls_image import Image, Image16, compile_blob
from test_directed_traffic_cpu import N, directed_batch, refused_v16_table, variant_options
from test_gpu_parity import VARIANTS, variant_acl
from test_gpu_rules import _check, to_device
from vpp_amd import _abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from vpp_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _hits(rules, tr, af=4):
    return oracle.classify_hits(oracle.rules_to_c(rules), tr["src"], tr["dst"], tr["dport"], tr["proto"], af=af)


def _img16(rules):
    return Image16(compile_blob(_abi.CRules(rules), "cls_compile_v16"))


# ---- 1, 2: the variant matrices ---------------------------------------------

@pytest.mark.parametrize("seed", range(2))
@pytest.mark.parametrize("kind", sorted(VARIANTS))
def test_rules_v4_variants(eng, libopt, kind, seed):
    """Every source lookup x list mode of the IPv4 classifier, LDS-resident,
    host arrays (the vector kernel of dispatch_slots4: at these sizes its
    leftover groups of four and its tail; its full-step loop is reached in
    test_gpu_classify_steps.py)."""
    for k, v in variant_options(kind, 4).items():
        libopt.set(k, v, eng)
    rules, pool = variant_acl(kind, seed)
    h = Image(compile_blob(_abi.CRules(rules))).h
    assert (h.mode, h.list_mode) == VARIANTS[kind], kind
    info = _check(eng, rules, directed_batch(rules, pool, seed))
    assert info["kernel"] == 1 and info["lds_resident"] == 1, info
    assert info["list_mode"] == VARIANTS[kind][1], info


@pytest.mark.parametrize("seed", range(2))
@pytest.mark.parametrize("kind", sorted(VARIANTS))
def test_rules_v16_variants(eng, libopt, kind, seed):
    """The mixed-family twins of the same tables: the core's list modes and
    source lookups behind the 16-byte front ends."""
    for k, v in variant_options(kind, 16).items():
        libopt.set(k, v, eng)
    rules, pool = variant_acl(kind, seed)
    rules, tr = mix_families(rules, directed_batch(rules, pool, seed), seed)
    info = _check(eng, rules, tr, af=16)
    assert info["has_v16"] == 1 and info["lds_resident_v16"] == 1, info


# ---- 3: the 16-byte front ends ----------------------------------------------

def _front_end_input(kind, seed):
    """The v4 / mixed / v16 inputs of test_v16_source_trie_on_gpu (IPv4 tables
    get a directed batch before they are widened), and `host`: the all-host-
    route sources that the source hashes (src_mode 1) are built for."""
    if kind == "v16":
        rules, pool = random_acl16(seed * 101 + 7, 150, 0.1, n_prefixes=60)
        return rules, random_traffic16(seed + 40, N, pool)
    if kind == "host":
        from test_cls16_cpu import _host_src_acl
        rules, pool = _host_src_acl(seed)
        return mix_families(rules, directed_traffic(rules, random_traffic(seed + 40, N, pool), seed), seed)
    rules, pool = random_acl(seed * 101 + 5, 150, 0.1, n_prefixes=80)
    tr = directed_traffic(rules, random_traffic(seed + 40, N, pool), seed)
    return mix_families(rules, tr, seed, 0.0 if kind == "v4" else 0.5)


@pytest.mark.parametrize("kind,option,src_mode", [
    ("v4", "v16_src_search", 0), ("mixed", "v16_src_search", 0), ("v16", "v16_src_search", 0),
    ("host", "v16_src_search", 0),
    ("v4", None, 0), ("mixed", None, 0), ("v16", None, 0), ("host", None, 1),
    ("v4", "v16_src_trie", 2), ("mixed", "v16_src_trie", 2), ("v16", "v16_src_trie", 2)])
def test_rules_v16_front_ends(eng, libopt, kind, option, src_mode):
    """src_mode 0 (interval search over 128-bit starts), 1 (host-route
    hashes) and 2 (IPv4 trie + non-IPv4 search): forced by option, or the
    compiler's own choice (fewer than 64 IPv4 source intervals: no trie)."""
    if option:
        libopt.set(option, "1", eng)
    rules, tr = _front_end_input(kind, 1)
    img = _img16(rules)
    assert img.core.has_cls and img.h.src_mode == src_mode
    info = _check(eng, rules, tr, af=16)
    assert info["has_v16"] == 1 and info["lds_resident_v16"] == 1, info


# ---- 4: source trie and wide cells ------------------------------------------

@pytest.mark.parametrize("af", [4, 16])
@pytest.mark.parametrize("seed", range(2))
@pytest.mark.parametrize("trie,wide", [("1", "0"), ("1", "1"), ("0", "1")])
def test_rules_trie_and_wide_cells(eng, libopt, trie, wide, seed, af):
    libopt.set("orient", "src", eng)
    libopt.set("trie", trie, eng)
    libopt.set("wide", wide, eng)
    rules, pool = single_port_acl(seed * 17 + 5, 200, n_prefixes=60)
    tr = directed_batch(rules, pool, seed)
    if af == 16:
        rules, tr = mix_families(rules, tr, seed)
        h = _img16(rules).core.h
    else:
        h = Image(compile_blob(_abi.CRules(rules))).h
        assert h.mode == (4 if trie == "1" else 0)
    if wide == "1":
        assert h.list_mode in (5, 6)
    info = _check(eng, rules, tr, af=af)
    assert info["lds_resident_v16" if af == 16 else "lds_resident"] == 1, info
    if af == 4:
        assert info["list_mode"] == h.list_mode


# ---- 5: counter tiers and the global-memory image ---------------------------

@pytest.mark.parametrize("tier", ["u16", "partial", "global"])
@pytest.mark.parametrize("table", ["random", "sublist"])
def test_rules_counter_tiers(eng, libopt, table, tier):
    """The images cls_classify counts on in u16 halves, with hot slots beside
    a partial LDS counter array (the slot -> rule map then has their extra
    entries), and from global memory (the kLds = false slot kernels)."""
    from test_gpu_counters import _budget, _layout
    rules, pool = random_acl(118, 400, 0.0) if table == "random" else single_port_acl(7, 300, n_prefixes=3)
    h = _layout(rules, libopt)
    assert h.has_cls
    libopt.set("lds_budget", str(_budget(h, tier)), eng)
    libopt.set("list_mode", str(h.list_mode), eng)
    libopt.set("trie", "1" if h.mode == 4 else "0", eng)
    libopt.set("orient", "src", eng)
    info = _check(eng, rules, directed_batch(rules, pool, 0))
    assert info["kernel"] == 1
    if tier == "global":
        assert info["lds_resident"] == 0, info
    else:
        assert info["lds_resident"] == 1 and info["ctr16"] == 1, info
        if tier == "partial":
            assert info["n_lctr"] < info["n_slots"], info
        else:
            assert info["n_lctr"] == info["n_slots"], info


def test_rules_v16_global_image(eng, libopt):
    libopt.set("lds_budget", "256", eng)
    rules, pool = random_acl(118, 400, 0.0)
    rules, tr = mix_families(rules, directed_batch(rules, pool, 0), 0)
    info = _check(eng, rules, tr, af=16)
    assert info["has_v16"] == 1 and info["lds_resident_v16"] == 0, info


# ---- 6: a table without a 16-byte classifier --------------------------------

def test_rules_refused_v16_table(eng):
    """32 nested IPv6 source networks are more than cls_compile_v16 has
    representatives for: the table has an IPv4 classifier only, and a 16-byte
    batch is CLS_E_INVAL for cls_classify_rules as it is for cls_classify.
    The engine and the table stay usable."""
    from vpp_amd.engine import ClsError
    rules, pool = refused_v16_table()
    t = eng.put_table("no16", rules)
    try:
        assert t.info()["has_v16"] == 0
        rules16, pool16 = random_acl16(5, 90, 0.0)
        tr16 = random_traffic16(2, N, pool16)
        with pytest.raises(ClsError, match="rc=%d: no 16-byte classifier" % _abi.E_INVAL):
            eng.classify(t, tr16["src"], tr16["dst"], tr16["dport"], tr16["proto"])
        with pytest.raises(ClsError, match="rc=%d: no 16-byte classifier" % _abi.E_INVAL):
            eng.classify_rules(t, tr16["src"], tr16["dst"], tr16["dport"], tr16["proto"])
        assert b"no 16-byte classifier" in _abi.lib().cls_last_error(eng.h)
        tr = directed_batch(rules, pool, 0)
        info = _check(eng, rules, tr, table=t)
        assert info["kernel"] == 1
        v, c = eng.classify(t, tr["src"], tr["dst"], tr["dport"], tr["proto"])
        ov, oc = oracle.classify_fast(oracle.rules_to_c(rules), tr["src"], tr["dst"], tr["dport"], tr["proto"])
        np.testing.assert_array_equal(v, ov)
        np.testing.assert_array_equal(c, oc)
        info = _check(eng, rules16, tr16, af=16)
        assert info["has_v16"] == 1
    finally:
        eng.del_table(t)


# ---- 7: device arrays and their alignment -----------------------------------

def _aligned_and_sliced(eng, rules, tr, af, table):
    """Aligned device tensors (the vector body), then the same tensors from
    element 1 on: IPv4 src / dst 4 bytes off their 16 (dispatch_slots4's
    one-packet-per-lane cases), dport 2 and proto 1 byte off; a row slice of
    the (n, 16) addresses stays 16-byte aligned.  Each with and without a
    verdict array."""
    dev = to_device(tr)
    assert all(d.data_ptr() % 16 == 0 for d in dev.values())
    want = _hits(rules, tr, af)
    for verdict in (True, False):
        _check(eng, rules, tr, af=af, table=table, want=want, dev=dev, verdict=verdict)
    sl = {k: v[1:] for k, v in tr.items()}
    sld = {k: d[1:] for k, d in dev.items()}
    assert sld["dport"].data_ptr() % 8 == 2 and sld["proto"].data_ptr() % 4 == 1
    assert sld["src"].data_ptr() % 16 == (0 if af == 16 else 4)
    for verdict in (True, False):
        _check(eng, rules, sl, af=af, table=table, want=(want[0][1:], want[1][1:]), dev=sld, verdict=verdict)


@pytest.mark.parametrize("kind,list_mode", [("hash_sph", 4), ("search_scan", 0)])
def test_rules_device_arrays_v4(eng, libopt, kind, list_mode):
    import torch
    from vpp_amd.engine import ClsError
    libopt.set("orient", "src", eng)
    libopt.set("list_mode", str(list_mode), eng)
    rules, pool = variant_acl(kind, 0)
    tr = directed_batch(rules, pool, 0)
    t = eng.put_table("dev", rules)
    try:
        info = t.info()
        assert info["kernel"] == 1 and info["lds_resident"] == 1 and info["list_mode"] == list_mode, info
        _aligned_and_sliced(eng, rules, tr, 4, t)
        # rule_out off its 4-byte alignment
        dev = to_device(tr)
        odd = torch.zeros(4 * N + 4, dtype=torch.uint8, device="cuda")[1:]
        with pytest.raises(ClsError, match="rc=%d: device arrays must be aligned" % _abi.E_INVAL):
            eng.classify_rules(t, dev["src"], dev["dst"], dev["dport"], dev["proto"], rules=odd)
        torch.cuda.synchronize()
    finally:
        eng.del_table(t)


def test_rules_device_arrays_v16(eng):
    import torch
    from vpp_amd.engine import ClsError
    rules, pool = random_acl16(41, 200, 0.0)
    tr = random_traffic16(6, N, pool)
    t = eng.put_table("dev16", rules)
    try:
        info = t.info()
        assert info["has_v16"] == 1 and info["lds_resident_v16"] == 1, info
        _aligned_and_sliced(eng, rules, tr, 16, t)
        dev = to_device(tr)
        odd = torch.zeros(4 * N + 4, dtype=torch.uint8, device="cuda")[1:]
        with pytest.raises(ClsError, match="rc=%d: device arrays must be aligned" % _abi.E_INVAL):
            eng.classify_rules(t, dev["src"], dev["dst"], dev["dport"], dev["proto"], rules=odd)
        torch.cuda.synchronize()
    finally:
        eng.del_table(t)


# ---- 8: batch-length edges ----------------------------------------------------

# around one vector group (4 packets per lane), one wave (64 lanes), one step
# of a wave in the 16-byte layout (4 x 64 packets), one workgroup (1024
# threads) and one step of it (4 x 1024)
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)


@pytest.mark.parametrize("af", [4, 16])
def test_rules_batch_length_edges(eng, libopt, af):
    """Prefixes of one directed batch on one imaged table, from host arrays
    and from aligned device tensors; a device call leaves the 64 elements
    after its outputs alone."""
    libopt.set("orient", "src", eng)
    rules, pool = variant_acl("hash_sph", 1)
    tr = directed_batch(rules, pool, 1)
    if af == 16:
        rules, tr = mix_families(rules, tr, 1)
    want = _hits(rules, tr, af)
    t = eng.put_table("edges", rules)
    try:
        info = t.info()
        assert info["kernel"] == 1 and info["lds_resident_v16" if af == 16 else "lds_resident"] == 1, info
        for n in LENGTHS:
            head = {k: v[:n] for k, v in tr.items()}
            w = (want[0][:n], want[1][:n])
            _check(eng, rules, head, af=af, table=t, want=w)
            _check(eng, rules, head, af=af, table=t, want=w, dev=to_device(head))
    finally:
        eng.del_table(t)


# ---- 9: the destination-keyed 16-byte image -----------------------------------

@pytest.mark.parametrize("orient", ["src", "dst"])
def test_rules_v16_destination_keyed(eng, libopt, orient):
    libopt.set("orient", orient, eng)
    rules, pool = random_acl(99, 300, 0.0)
    rules, tr = mix_families(rules, directed_batch(rules, pool, 5), 5)
    assert _img16(rules).core.h.swap == (1 if orient == "dst" else 0)
    info = _check(eng, rules, tr, af=16)
    assert info["has_v16"] == 1 and info["lds_resident_v16"] == 1, info
