"""Traffic aimed at the rules (aclgen.directed_traffic), checked on the CPU.

random_traffic draws addresses around the pool's prefixes and ports from a
short list, so on the tables with many port ranges (bit vectors with per-list
port search) and with long candidate lists (template scan) nearly every
packet ends at the default DENY, and a parity test over such a batch mostly
asserts that a kernel returns DENY.  directed_traffic aims about three
quarters of a batch at the rules themselves.  The conditions below are
asserted on the oracle alone (orc_classify_fast_hits, pinned to evalACL in
test_oracle_pin_cpu.py): they state what the GPU tests built on these batches
(test_gpu_rules_variants.py, the second batch of the classify matrices) get to
see -- few default DENYs, many distinct terminating rules, every action.

On the same batches the CPU interpreters of the compiled blobs
(tests/cls_image.py) equal the oracle, verdicts and counters, under the
options that pin each variant; and the table of 32 nested IPv6 source
networks that the 16-byte compiler refuses (no room for its representatives)
is refused by cls_compile_v16 alone.
"""
import numpy as np
import pytest

import oracle
from aclgen import directed_traffic, mix_families, random_acl, random_traffic, single_port_acl
from cls_image import Image, Image16, compile_blob
from test_gpu_parity import VARIANTS, variant_acl
from vpp_amd import _abi
from vpp_amd import model as M

N = 4099


def variant_options(kind, af=4):
    """The library switches under which test_all_kernel_variants (af 4) and
    test_v16_all_kernel_variants (af 16) compile variant_acl(kind, seed)."""
    opts = {"trie": "1" if kind.startswith("trie") else "0"}
    if kind.endswith("_pc"):
        opts["list_mode_max"] = "2"
    if af == 4:
        opts["orient"] = "src"
        opts["src_search"] = "1" if kind.startswith(("search", "trie")) else "0"
    return opts


def directed_batch(rules, pool, seed, n=N):
    return directed_traffic(rules, random_traffic(seed + 11, n, pool), seed)


def nested_v6_rules(last=64):
    """Sources 2001:db8::/33 .. /last, each inside the one before: at /64 one
    more nesting level than cls_compile_v16 has representatives for."""
    return [M.l4_rule(M.PERMIT, "2001:db8::/%d" % k, "", "tcp", 0, 65535, 80, 80) for k in range(33, last + 1)]


def refused_v16_table():
    """A table with an IPv4 classifier and no 16-byte one."""
    rules, pool = random_acl(3, 40, 0.0)
    return nested_v6_rules() + rules, pool


def _tables():
    out = [("%s-%d" % (kind, seed), kind, seed) for kind in sorted(VARIANTS) for seed in (0, 1)]
    out += [("trie_wide-%d" % seed, None, seed) for seed in (0, 1)]
    out += [("tiers_random", None, 0), ("tiers_sublist", None, 0), ("refused_v16", None, 0)]
    return out


def _table(name, kind, seed):
    if kind is not None:
        return variant_acl(kind, seed)
    if name.startswith("trie_wide"):
        return single_port_acl(seed * 17 + 5, 200, n_prefixes=60)
    if name == "tiers_random":
        return random_acl(118, 400, 0.0)
    if name == "tiers_sublist":
        return single_port_acl(7, 300, n_prefixes=3)
    return refused_v16_table()


def _premise(rules, tr, af, max_default):
    ov, oh = oracle.classify_hits(oracle.rules_to_c(rules), tr["src"], tr["dst"], tr["dport"], tr["proto"], af=af)
    R = len(rules)
    share = float((oh == R).mean())
    distinct = len(np.unique(oh[oh < R]))
    print("af %d: default DENY %.3f, %d distinct terminating rules, actions %s" % (
        af, share, distinct, np.unique(ov).tolist()))
    assert share <= max_default
    assert distinct >= 10
    assert set(np.unique(ov).tolist()) >= {M.DENY, M.PERMIT, M.REFLECT}
    return ov, np.bincount(oh, minlength=R + 1).astype(np.uint64)


@pytest.mark.parametrize("name,kind,seed", _tables(), ids=[t[0] for t in _tables()])
def test_directed_batches_reach_the_rules(name, kind, seed, libopt):
    """The premise, on the oracle; then the interpreters of both layouts'
    blobs on the same batches, under the variant's options."""
    rules, pool = _table(name, kind, seed)
    tr = directed_batch(rules, pool, seed)
    ov, oc = _premise(rules, tr, 4, 0.5)
    rules16, tr16 = mix_families(rules, tr, seed)
    ov16, oc16 = _premise(rules16, tr16, 16, 0.9)

    for k, v in (variant_options(kind, 4) if kind else {"orient": "src"}).items():
        libopt.set(k, v)
    img = Image(compile_blob(_abi.CRules(rules)))
    if kind:
        assert (img.h.mode, img.h.list_mode) == VARIANTS[kind]
    v, c = img.classify(tr["src"], tr["dst"], tr["dport"], tr["proto"])
    np.testing.assert_array_equal(v, ov)
    np.testing.assert_array_equal(c, oc)

    if name == "refused_v16":
        return
    libopt.undo()
    for k, v in (variant_options(kind, 16) if kind else {}).items():
        libopt.set(k, v)
    img16 = Image16(compile_blob(_abi.CRules(rules16), "cls_compile_v16"))
    v, c = img16.classify(tr16["src"], tr16["dst"], tr16["dport"], tr16["proto"])
    np.testing.assert_array_equal(v, ov16)
    np.testing.assert_array_equal(c, oc16)


def test_directed_traffic_is_deterministic_and_keeps_the_rest():
    rules, pool = random_acl(5, 80, 0.2)
    base = random_traffic(3, N, pool)
    a, b = directed_traffic(rules, base, 9), directed_traffic(rules, base, 9)
    for k in base:
        np.testing.assert_array_equal(a[k], b[k])
        assert a[k].dtype == base[k].dtype and a[k] is not base[k]
    other = directed_traffic(rules, base, 10)
    assert any((a[k] != other[k]).any() for k in ("src", "dst", "dport"))
    # an aimed packet gets protocol 0..2: every protocol > 2 of the batch is one of the base's
    assert (base["proto"][a["proto"] > 2] == a["proto"][a["proto"] > 2]).all()
    assert (a["proto"] > 2).any()
    same = np.ones(N, bool)
    for k in ("src", "dst", "dport", "proto"):
        same &= a[k] == base[k]
    assert 0.15 < same.mean() < 0.45                       # about 1 - share untouched (malformed rules add a few)
    none = directed_traffic(rules, base, 9, share=0.0)
    for k in base:
        np.testing.assert_array_equal(none[k], base[k])


def test_nested_v6_sources_refused_by_v16_compiler_only():
    rules, _ = refused_v16_table()
    with pytest.raises(RuntimeError, match="cls_compile_v16 rc=%d" % _abi.E_INVAL):
        compile_blob(_abi.CRules(rules), "cls_compile_v16")
    assert Image(compile_blob(_abi.CRules(rules))).h.n_rules == len(rules)
    ok = nested_v6_rules(63) + rules[32:]
    assert Image16(compile_blob(_abi.CRules(ok), "cls_compile_v16")).core.h.n_rules == len(ok)
