"""CPU: the batch-size census, the depth generators and the traffic of the
full-step-loop tests (tests/classify_steps_cases.py, used on the GPU by
tests/test_gpu_classify_steps.py).

The census functions equal a literal thread-by-thread simulation of the
kernels' loops; the suite's older parity batch sizes never reach
classify4_cls's full-step loop; every generator compiles to the (source
mode, list mode, depth) it declares, in the main, the pair and the 16-byte
image; the CPU interpreter of those images equals the evalACL oracle; and
the oracle alone shows that each batch reaches every rung's rule and the
default DENY inside the full-step loop.
"""
import numpy as np
import pytest

import classify_steps_cases as K
import oracle
from cls_image import Image, Image16, compile_blob
from vpp_amd import _abi

N_CU = 256            # MI355X; the GPU tests read the device's


@pytest.mark.parametrize("cus", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("lds", [True, False])
def test_census4_equals_the_simulated_loops(cus, lds):
    """Grids of 1 to 10 workgroups at a block of 8 threads: every n up to
    three rounds of the largest grid, and past it."""
    block = 8
    top = cus * K.per_cu(lds)
    for n in range(0, 4 * block * top * 3 + 4 * block + 7):
        grid, rounds, left, tail = K.census4(n, cus, lds, block=block)
        assert 1 <= grid <= top
        full, lo, t = K.simulate4(n, grid, block)
        assert len(full) == 4 * rounds * grid * block, n
        assert (len(lo), len(t)) == (4 * left, tail), n
        assert full + lo + t == list(range(n)), n         # every packet once, the loops in index order


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 12288, 12288 + 23, 3 * 4096 * 2 + 4 * 777 + 3])
def test_census4_spot_checks_at_the_real_block(n):
    grid, rounds, left, tail = K.census4(n, 3, True)
    full, lo, t = K.simulate4(n, grid)
    assert (len(full), len(lo), len(t)) == (4096 * grid * rounds, 4 * left, tail)
    assert full + lo + t == list(range(n))


def test_wg_per_cu_option():
    assert K.census4(1 << 22, 256, True, wg_per_cu=2)[0] == 512
    assert K.census4(1 << 22, 256, False, wg_per_cu=1)[0] == 256
    assert K.census4(1 << 22, 256, False, wg_per_cu=7)[0] == 512


@pytest.mark.parametrize("cus", [1, 3])
def test_census16_equals_the_simulated_loops(cus):
    block = 64
    for n in list(range(0, 256 * 3 * 3 + 300, 7)) + [256 * 23 + 119]:
        grid, steps, tail = K.census16(n, cus, True, block=block)
        st, t = K.simulate16(n, grid, block)
        assert (len(st), len(t)) == (256 * steps, tail)
        assert st + t == list(range(n))
    grid, steps, tail = K.census16(256 * 23 + 119, 256, True)
    st, t = K.simulate16(256 * 23 + 119, grid)
    assert (grid, len(st), len(t)) == (2, 256 * 23, 119) and (steps, tail) == (23, 119)


@pytest.mark.parametrize("file,n", [(f, n) for f, ns in sorted(K.SUITE_SIZES.items()) for n in ns])
@pytest.mark.parametrize("lds", [True, False])
def test_older_parity_batches_never_reach_the_full_step_loop(file, n, lds):
    grid, rounds, left, tail = K.census4(n, N_CU, lds)
    assert rounds == 0 and 4 * left + tail == n


def test_batch_size_builders():
    for g in (1, 2, 3, 200):
        assert K.census4(K.one_round(g), N_CU, True) == (g, 1, 0, 0)
        assert K.census4(K.one_round(g), N_CU, False) == (g, 1, 0, 0)
    assert K.census4(K.one_round(3) + 4 * 5 + 3, N_CU, True) == (4, 0, 3 * 1024 + 5, 3)
    for cus, pcu, rounds in ((256, 1, 1), (256, 2, 1), (256, 1, 2), (304, 1, 1), (7, 2, 3)):
        n = K.saturated(cus, pcu, rounds, 777, 3)
        assert K.census4(n, cus, pcu == 1) == (cus * pcu, rounds, 777, 3)
    assert K.saturated(256, 2, 1, 777, 3) <= int(2.1 * (1 << 20))


def _compile(case, fn="cls_compile_v4", rules=None, **extra):
    opts = {k: str(v) for k, v in case.options.items()}
    opts.update({k: str(v) for k, v in extra.items()})
    return compile_blob(_abi.CRules(case.rules if rules is None else rules), fn, options=opts)


@pytest.mark.parametrize("depth,lookup,list_mode", K.DEPTH_CASES)
def test_generators_reach_what_they_declare(depth, lookup, list_mode):
    """Main image, pair image (option pair4) and the CPU interpreter against
    the oracle, the coverage condition on the batch the GPU depth test sends."""
    c = K.for_depth(depth, lookup, list_mode)
    assert len(c.rules) >= 64
    img = Image(_compile(c))
    h = img.h
    assert h.has_cls and (h.mode, h.list_mode, h.bv_steps_d) == (c.mode, c.list_mode, c.depth) == \
        (K.LOOKUPS[lookup][1], list_mode, depth), c
    assert (h.n_hash == 1) == (c.variant == 2)            # the one-length hash kernel
    assert h.ctr16 == 0                                   # u32 LDS counters: the depth-specialised launch
    hp = Image(_compile(c, pair4=1)).h
    assert (hp.mode, hp.list_mode, hp.bv_steps_d) == (c.mode, c.list_mode, c.depth), c
    n = K.one_round(2)
    assert K.census4(n, N_CU, True) == (2, 1, 0, 0)
    tr = K.ladder_traffic(c, n, other_every=16)
    want = oracle.classify_faithful(oracle.rules_to_c(c.rules), tr["src"], tr["dst"], tr["dport"], tr["proto"])
    got = img.classify(tr["src"], tr["dst"], tr["dport"], tr["proto"])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert K.reached(c, tr, n)
    assert len(set(want[0].tolist())) == 3                # DENY, PERMIT and REFLECT all seen


def test_ladder_depth_formula():
    assert [K.ladder_depth(m) for m in (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)] == [2, 3, 3, 4, 4, 5, 5, 6, 6, 6, 7]
    for d, m in K.M_OF_DEPTH.items():
        assert K.ladder_depth(m) == d == K.ladder(m).depth


@pytest.mark.parametrize("m", [3, 4, 8, 16, 31])
def test_ladders_between_the_named_ones_compile_to_the_formula(m):
    c = K.ladder(m)
    h = Image(_compile(c)).h
    assert (h.list_mode, h.bv_steps_d) == (4, K.ladder_depth(m))


def test_a_longer_ladder_leaves_the_sublist_modes():
    c = K.ladder(33)
    h = Image(_compile(c)).h
    assert h.has_cls and h.list_mode == 0


@pytest.mark.parametrize("key", sorted(K.TWINS))
@pytest.mark.parametrize("fe,lookup,opts", [(0, "hash", {"v16_src_search": 1}), (1, "host", {}),
                                            (2, "hash", {"v16_src_trie": 1})])
def test_twins_reach_their_depth_in_the_16_byte_layout(key, fe, lookup, opts):
    """The mixed-family twins: core depth, front end, the interpreter of the
    16-byte image against the oracle (on a batch with a per-packet tail), and
    the coverage condition over the wave-steps."""
    n = 256 * 7 + 119
    c, rules, tr, depth = K.twin(key, lookup, n, other_every=16)
    blob = compile_blob(_abi.CRules(rules), "cls_compile_v16", options=dict({"orient": "src"}, **opts))
    img = Image16(blob)
    assert img.h.core.has_cls and (img.h.core.list_mode, img.h.core.bv_steps_d, img.h.src_mode) == (4, depth, fe)
    hp = Image16(compile_blob(_abi.CRules(rules), "cls_compile_v16",
                              options=dict({"orient": "src", "pair4": 1}, **opts))).h
    assert (hp.core.list_mode, hp.core.bv_steps_d, hp.src_mode) == (4, depth, fe)
    want = oracle.classify_faithful(oracle.rules_to_c(rules), tr["src"], tr["dst"], tr["dport"], tr["proto"], af=16)
    got = img.classify(tr["src"], tr["dst"], tr["dport"], tr["proto"])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert K.reached(c, tr, 256 * 7, af=16)


@pytest.mark.parametrize("key", ["flat0", "ladder9", "ladder17", "search", "host", "trie"])
@pytest.mark.parametrize("pcu,rounds", [(1, 1), (2, 1), (1, 2)])
def test_saturated_batches_reach_every_rung_in_the_full_step_loop(key, pcu, rounds):
    c = K.saturated_case(key)
    n = K.saturated(N_CU, pcu, rounds, 777, 3)
    grid, r, left, tail = K.census4(n, N_CU, pcu == 1)
    assert (grid, r, left, tail) == (N_CU * pcu, rounds, 777, 3)
    tr = K.ladder_traffic(c, n, other_every=10)
    nfull = r * grid * K.BLOCK
    assert K.reached(c, tr, 4 * nfull)
    # and the two short loops see packets that reach a rule, not only the default DENY
    _, hits = oracle.classify_hits(oracle.rules_to_c(c.rules), tr["src"], tr["dst"], tr["dport"], tr["proto"])
    assert (hits[4 * nfull:n - tail] < len(c.rules)).any() and len(set(hits[4 * nfull:].tolist())) > 3
