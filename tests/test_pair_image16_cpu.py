"""The 16-byte connection pair launch's four-cell image (CPU).

classify16_pair (vpp_amd/csrc/k16_pair.hip) classifies both tuples of every
connection of a mixed-family batch on the 16-byte image with a fourth cell
per source class for protocols > 2 (compile.hpp build_pair16; cls_compile_v16
option pair4), instead of the main image plus the OTHER image.  Here that
compile is checked without a GPU: the blob keeps the layout
cls_image_v16_header describes (tests/cls_image.py Image16 decodes it
unchanged: front-end tables, source-search trailer), has no OTHER image,
every index the core and the front end hand the kernel is in range
(test_image_ranges_cpu's walk), and the image evaluated as the kernel reads
it (min(protocol, 3) picks the cell; src_mode 1 and 2 go from the front end's
row straight to it) gives evalACL's verdict and terminating rule for TCP,
UDP, ICMP and other protocol values against the faithful oracle
(classify_faithful, af=16).  Bit-exact verdicts and per-rule counts; a fifth
of every batch is on protocols 3, 6, 17, 47 and 255.
"""
import numpy as np
import pytest

import oracle
from aclgen import (long_list_acl, many_ports_acl, mix_families, random_acl16, random_traffic, random_traffic16,
                    single_port_acl)
from cls_image import Image16, compile_blob
from test_image_ranges_cpu import check_image
from vpp_amd import _abi


def _image16(rules, **opts):
    return Image16(compile_blob(_abi.CRules(rules), "cls_compile_v16", options=opts or None))


def _with_other_protocols(tr, seed, frac=0.2):
    rng = np.random.default_rng(seed)
    other = rng.random(len(tr["proto"])) < frac
    tr = dict(tr)
    tr["proto"] = np.where(other, rng.choice(np.array([3, 6, 17, 47, 255], np.uint8), len(other)),
                           tr["proto"]).astype(np.uint8)
    assert (tr["proto"] > 2).mean() > 0.15
    return tr


def _check_front_end(im, main, blob_len):
    """The front end is the main image's (same modes and table shapes), and
    every row it can hand the core is a class row of the four-cell core."""
    h, c = im.h, im.core.h
    assert h.src_mode == main.h.src_mode
    assert c.swap == main.core.h.swap
    assert [h.fe_top[1], h.fe_n[1], h.fe_k8[1]] == [main.h.fe_top[1], main.h.fe_n[1], main.h.fe_k8[1]]
    assert c.mode == (3 if h.src_mode else c.mode) and c.row_bytes == im.core.ncell * (8 if c.list_mode in (0, 5, 6) else 4)

    def rows_ok(rows):
        rows = np.asarray(rows, np.int64)
        assert ((rows - c.off_cells) % c.row_bytes == 0).all(), "front-end row not a class row"
        assert ((rows >= c.off_cells) & ((rows - c.off_cells) // c.row_bytes < c.n_classes)).all(), "row past n_classes"

    for sd in range(2):
        if sd == 0 and h.src_mode == 1:
            continue                                   # (side 0's table is the trailer's, reps)
        end = h.fe_val[sd] + 4 * h.fe_n[sd]
        assert h.fe_key[sd] + (8 if h.fe_k8[sd] else 16) * h.fe_top[sd] <= h.fe_val[sd] and end <= c.img_bytes
    if h.src_mode == 2:                                # the non-IPv4 search's values are rows
        rows_ok(im.vals[0])
    if h.src_mode == 1:
        rows_ok([h.dflt_row[0], h.dflt_row[1]])
        img = im._img
        t4 = np.frombuffer(img, np.uint32, count=4 * h.cap4, offset=h.h4).reshape(-1, 2)
        k6 = np.frombuffer(img, np.uint32, count=8 * h.cap6, offset=h.k6).reshape(-1, 4)
        r6 = np.frombuffer(img, np.uint32, count=2 * h.cap6, offset=h.r6)
        # (an empty slot's key never probes it and its row stays 0: only rows a probe can return)
        rows_ok(t4[t4[:, 1] != 0, 1])
        rows_ok(r6[r6 != 0])
        assert h.r6 + 8 * h.cap6 <= c.img_bytes and len(k6) == 2 * h.cap6
    if h.src_mode:
        assert h.off_src_search and h.off_src_search + h.src_search_val <= blob_len   # the trailer stays


def _check(rules, tr, **opts):
    main = _image16(rules, **opts)
    assert main.core.has_cls                           # the main compile has a classifier (nothing skipped)
    blob = compile_blob(_abi.CRules(rules), "cls_compile_v16", options=dict(opts, pair4=1))
    im = Image16(blob)
    assert im.core.has_cls
    assert im.core.ncell == 4, im.core.ncell
    assert im.core.other is None and im.core.h.off_other == 0
    check_image(im.core, len(rules))
    _check_front_end(im, main, len(blob))
    v, c = im.classify(tr["src"], tr["dst"], tr["dport"], tr["proto"])
    ov, oc = oracle.classify_faithful(oracle.rules_to_c(rules), tr["src"], tr["dst"], tr["dport"], tr["proto"],
                                      af=16)
    bad = np.nonzero(v != ov)[0]
    assert bad.size == 0, (bad[:8], v[bad[:8]], ov[bad[:8]], tr["proto"][bad[:8]])
    np.testing.assert_array_equal(c, oc)
    return im


def _config_twin(cfg, n):
    from vpp_amd import workload
    acl, spec, _ = workload.config(cfg)
    tr = oracle.gen_traffic_v4(spec, 5, n)
    return mix_families(acl.rules, tr, cfg)


def test_pair_image16_config2_twin():
    """The mixed-family twin of the rendered config-2 table (the GPU tests'
    global ACL): host-route sources, rows from the hashes."""
    rules, tr = _config_twin(2, 20000)
    im = _check(rules, _with_other_protocols(tr, 2))
    assert im.h.src_mode == 1 and im.core.h.mode == 3


def test_pair_image16_config5():
    """The config-5 render on its own 16-byte stream."""
    from vpp_amd import workload
    acl, spec, _ = workload.config(5)
    tr = oracle.gen_traffic_v16(spec, 0, 5000)
    im = _check(acl.rules, _with_other_protocols(tr, 5))
    assert im.h.src_mode == 1 and im.core.h.mode == 3


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("n_rules,weird", [(70, 0.0), (150, 0.05), (300, 0.15)])
def test_pair_image16_random_acls(seed, n_rules, weird):
    """Random mixed-family ACLs with malformed rules: the interval-search
    front end (reps through the core's own source lookup)."""
    rules, pool = random_acl16(seed * 1000 + n_rules, n_rules, weird)
    tr = _with_other_protocols(random_traffic16(seed, 1500, pool), seed + n_rules)
    im = _check(rules, tr)
    assert im.h.src_mode in (0, 1)
    if im.h.src_mode == 0:
        assert im.core.h.mode in (0, 1, 4)


def _twins(s):
    return [single_port_acl(s + 3, 200), many_ports_acl(s, 300, 30), long_list_acl(s + 1, 250)]


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("variant", ["plain", "dst", "trie"])
def test_pair_image16_twins_front_ends_and_orientation(s, variant):
    """Twins of IPv4 tables as they compile, destination-keyed (orient=dst:
    swap 1) and with the IPv4 source trie (v16_src_trie=1: src_mode 2 unless
    every source is a host route)."""
    opts = {"plain": {}, "dst": {"orient": "dst"}, "trie": {"v16_src_trie": 1}}[variant]
    modes = []
    for k, (rules, pool) in enumerate(_twins(s)):
        rules, tr = mix_families(rules, random_traffic(s * 7 + k, 2500, pool), s + k)
        im = _check(rules, _with_other_protocols(tr, s + k), **opts)
        modes.append(im.h.src_mode)
        if variant == "dst":
            assert im.core.h.swap == 1
        if variant == "trie":
            assert im.h.src_mode in (1, 2)
    if variant == "trie":
        assert modes[0] == 2, modes                    # the single-port tables' sources are not all host routes


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("cap", [0, 1, 2, 3, 4])
def test_pair_image16_twins_every_list_mode(s, cap):
    for k, (rules, pool) in enumerate(_twins(s)):
        rules, tr = mix_families(rules, random_traffic(s * 7 + k, 2000, pool), s + k)
        im = _check(rules, _with_other_protocols(tr, s + k + cap), list_mode_max=cap)
        assert im.core.h.list_mode <= cap


def test_pair_image16_follows_the_main_orientation():
    """The pair launch frames both tuples once, so the pair image takes the
    main image's orientation under both forced orientations."""
    rules, pool = random_acl16(99, 300, 0.0)
    tr = _with_other_protocols(random_traffic16(5, 2000, pool), 5)
    for orient, swap in (("dst", 1), ("src", 0)):
        main = _image16(rules, orient=orient)
        im = _check(rules, tr, orient=orient)
        assert main.core.h.swap == swap and im.core.h.swap == main.core.h.swap
