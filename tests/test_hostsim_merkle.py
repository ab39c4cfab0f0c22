"""CPU tier: the Merkle kernels in every form -- one parent per lane (k_merkle_level_fast), five waves per parent
(k_merkle_coop, single level and the fused multi-level run), one parent per wave (k_merkle_lanes, helped and not) and per
16-lane row (k_merkle_rows), open, verify and update in their forms -- through the shipped size dispatch and merkle_run,
under ASan+UBSan, byte for byte against the oracle.  The sizes are the smallest that reach each form (tests/gpu_common.py
FORM_SIZES / LEVEL_SIZES), and for the DPP forms of hades_lanes.hpp the smallest that reach every role of a block.

A block of a DPP form costs seconds here (tests/hostsim/hip/hip_runtime.h), and every tree of more than 4 096 parents
ends in a thousand of them.  So whole trees, roots and updates are compared in full on SMALL trees (every level a DPP
form), and the trees that reach the per-lane and five-waves levels run with HOSTSIM_DPP_MAX_BLOCKS=0: the launches of
their small levels are given up and reported, and the levels above are compared with the oracle's tree."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostsim_lib as HS  # noqa: E402
import oracle_lib  # noqa: E402
from oracle_lib import limbs_of  # noqa: E402
from gpu_common import TAG, edge_scalars, level_form, verify_form, update_form, FORM_SIZES, LEVEL_SIZES  # noqa: E402


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def u64(b):
    return np.frombuffer(b, dtype=np.uint64)


def tag_buf(s, arity):
    return s.buf("tag%d" % arity, np.array(limbs_of(TAG[arity]), dtype=np.uint64).tobytes())


@pytest.mark.parametrize("arity,n_children,padded", [(2, 2 * 16385, False), (4, 4 * 4097 + 1, True), (3, 3 * 4097 + 2, False),
                                                     (1, 4097 * 4 + 1, False)])
def test_level_one_parent_per_lane(oracle, arity, n_children, padded):
    """Full levels above 16 384 parents and ragged ones above 4 096, with and without a padding digest."""
    assert level_form(n_children, arity) == "k_merkle_level_fast<%d>" % arity
    n_parents = -(-n_children // arity)
    ch = edge_scalars(n_children, 40 + arity)
    pad = edge_scalars(1, 99) if padded else None
    s = HS.Script("merkle")
    s.buf("ch", ch.tobytes())
    s.fill("par", 32 * n_parents, 0xFF)
    if padded:
        s.buf("pad", pad.tobytes())
    s.call("hades252_merkle_level_pad_dev", "ch", n_children, "par", arity, tag_buf(s, arity), 1, "pad" if padded else None,
           None)
    s.dump("par")
    r = s.run(timeout=600)                               # measured: 2 s (4 098 parents) .. 6 s (16 386)
    assert r.rc == [("hades252_merkle_level_pad_dev", 0)]
    assert (u64(r.out["par"]) == oracle.merkle_level_pad(ch, arity, TAG[arity], 1, pad)).all()


@pytest.mark.parametrize("arity", [2, 4])                 # (arity 3: the second level of test_root_only_ping_pong_buffers)
def test_level_five_waves_per_parent(oracle, arity):
    n_parents = LEVEL_SIZES["coop"][0]                    # 4 097: 65 blocks, one parent in the last
    assert level_form(arity * n_parents, arity) == "k_merkle_coop<%d>" % arity
    ch = edge_scalars(arity * n_parents, 50 + arity)
    s = HS.Script("merkle")
    s.buf("ch", ch.tobytes())
    s.fill("par", 32 * n_parents, 0xFF)
    if arity == 4:
        s.call("hades252_merkle4_level_dev", "ch", "par", n_parents, tag_buf(s, arity), 1, None)
    else:
        s.call("hades252_merkle_level_dev", "ch", "par", n_parents, arity, tag_buf(s, arity), 1, None)
    s.dump("par")
    r = s.run(timeout=900)                               # measured: 10 s
    assert [rc for _, rc in r.rc] == [0]
    assert (u64(r.out["par"]) == oracle.merkle_level(ch, arity, TAG[arity], 1)).all()


def run_tree(oracle, arity, n_leaves, padded, seed):
    """hades252_merkle_build[_pad]_dev -> (result, oracle levels, byte offset of each level in the tree)."""
    leaves = edge_scalars(n_leaves, seed)
    depth = 0
    n = n_leaves
    while n > 1:
        n = -(-n // arity)
        depth += 1
    pad = edge_scalars(depth, seed + 1).reshape(depth, 4) if padded else None
    levels = oracle.merkle_tree(leaves, arity, TAG[arity], 1, pad)
    tree_bytes = 8 * sum(l.size for l in levels)
    s = HS.Script("merkle")
    s.buf("leaves", leaves.tobytes())
    s.fill("tree", tree_bytes, 0xFF)
    s.call("hades252_merkle_tree_bytes", n_leaves, arity)
    if padded:
        s.buf("pad", pad.tobytes())
        s.call("hades252_merkle_build_pad_dev", "leaves", n_leaves, arity, tag_buf(s, arity), 1, "pad", "tree", None)
    else:
        s.call("hades252_merkle_build_dev", "leaves", n_leaves, arity, tag_buf(s, arity), 1, "tree", None)
    s.dump("tree")
    return s, leaves, levels, pad, tree_bytes


def check_large_levels(r, levels, tree_bytes, n_emulated):
    """The first n_emulated levels are the oracle's; every later launch is a DPP form over the block budget and was given up."""
    assert r.rc[0] == ("hades252_merkle_tree_bytes", tree_bytes) and r.rc[1][1] == 0
    tree = u64(r.out["tree"])
    off = 0
    for l, lev in enumerate(levels[:n_emulated]):
        assert (tree[off:off + lev.size] == lev).all(), "level %d" % (l + 1)
        off += lev.size
    assert "over_budget hades252_merkle_build" in r.stdout
    assert (tree[off:] == 0xFFFFFFFFFFFFFFFF).all()       # nothing else wrote into the tree


def test_whole_tree_ragged_with_padding_table(oracle, monkeypatch):
    """merkle_run, arity 4, 65 543 leaves: 16 386 parents (per lane), then 4 097 from a ragged level (per lane, pad[1]);
    the 1 025-parent level and the ones above it are DPP forms over the block budget (the small trees below run those)."""
    monkeypatch.setenv("HOSTSIM_DPP_MAX_BLOCKS", "0")
    s, leaves, levels, pad, tree_bytes = run_tree(oracle, 4, 4 * 16385 + 3, True, 60)
    assert [l.size // 4 for l in levels[:3]] == [16386, 4097, 1025]
    r = s.run(timeout=900)                               # measured: 9 s
    check_large_levels(r, levels, tree_bytes, 2)


def test_whole_tree_fused_coop_levels(oracle, monkeypatch):
    """merkle_run, arity 2, 2^15 leaves: the levels of 16 384 and 8 192 parents are ONE k_merkle_coop launch (n_levels = 2,
    64 parents per block through two levels in LDS) -- the only shape the fusion rule of merkle_run admits below the DPP
    forms' sizes."""
    monkeypatch.setenv("HOSTSIM_DPP_MAX_BLOCKS", "0")
    s, leaves, levels, pad, tree_bytes = run_tree(oracle, 2, 1 << 15, False, 61)
    r = s.run(timeout=1800)                              # measured: 50 s (256 blocks of 320 threads, 2 x 67 barriers each)
    check_large_levels(r, levels, tree_bytes, 2)


@pytest.mark.parametrize("entry,arity,n_leaves", [("hades252_merkle_root_pad_dev", 4, 4 * 16385 + 3),
                                                  ("hades252_merkle_root_dev", 3, 3 * 16385 + 1),
                                                  ("hades252_merkle4_root_dev", 4, 4 * 16385 + 3)])
def test_root_only_ping_pong_buffers(oracle, monkeypatch, entry, arity, n_leaves):
    """merkle_run without a tree: level 1 lands in the first scratch buffer, level 2 in the second (per lane, per lane from
    a ragged level or five waves per parent); the third level is a DPP form over the block budget."""
    monkeypatch.setenv("HOSTSIM_DPP_MAX_BLOCKS", "0")
    leaves = edge_scalars(n_leaves, 65)
    padded = entry.endswith("_pad_dev")
    depth, n = 0, n_leaves
    while n > 1:
        n = -(-n // arity)
        depth += 1
    pad = edge_scalars(depth, 66).reshape(depth, 4) if padded else None
    levels = oracle.merkle_tree(leaves, arity, TAG[arity], 1, pad)
    n1, n2 = levels[0].size // 4, levels[1].size // 4
    assert n1 > 16384 and 4096 < n2 <= 16384 and levels[2].size // 4 <= 4096
    s = HS.Script("merkle")
    s.buf("leaves", leaves.tobytes())
    s.fill("scratch", 32 * (n1 + n2), 0xFF)
    s.fill("root", 32, 0xFF)
    s.call("hades252_merkle_scratch_bytes", n_leaves, arity)
    if padded:
        s.buf("pad", pad.tobytes())
        s.call(entry, "leaves", n_leaves, arity, "scratch", 32 * (n1 + n2), tag_buf(s, arity), 1, "pad", "root", None)
    elif entry == "hades252_merkle4_root_dev":
        s.call(entry, "leaves", n_leaves, "scratch", 32 * (n1 + n2), tag_buf(s, arity), 1, "root", None)
    else:
        s.call(entry, "leaves", n_leaves, arity, "scratch", 32 * (n1 + n2), tag_buf(s, arity), 1, "root", None)
    s.dump("scratch")
    r = s.run(timeout=900)                               # measured: 9 s (per-lane levels) / 20 s (a five-waves second level)
    assert r.rc == [("hades252_merkle_scratch_bytes", 32 * (n1 + n2)), (entry, 0)]
    scratch = u64(r.out["scratch"])
    assert (scratch[:4 * n1] == levels[0]).all() and (scratch[4 * n1:] == levels[1]).all()
    assert "over_budget " + entry in r.stdout


def test_forest_of_two_leaf_trees(oracle):
    """hades252_merkle_forest_dev: 16 385 trees of 2 leaves = one per-lane level, the roots contiguous."""
    n = FORM_SIZES["fast"][0]
    leaves = edge_scalars(2 * n, 62)
    s = HS.Script("merkle")
    s.buf("leaves", leaves.tobytes())
    s.fill("roots", 32 * n, 0xFF)
    s.call("hades252_merkle_forest_scratch_bytes", n, 2, 2)
    s.call("hades252_merkle_forest_dev", "leaves", n, 2, 2, None, 0, tag_buf(s, 2), 1, "roots", None)
    s.dump("roots")
    r = s.run(timeout=600)                               # measured: 5 s
    assert [rc for _, rc in r.rc] == [0, 0]
    assert (u64(r.out["roots"]) == oracle.merkle_level(leaves, 2, TAG[2], 1)).all()


def expected_paths(leaves, levels, arity, indices, pad):
    nodes = [leaves.reshape(-1, 4)] + [l.reshape(-1, 4) for l in levels[:-1]]
    depth = len(levels)
    out = np.zeros((len(indices), depth, arity - 1, 4), dtype=np.uint64)
    for t, idx in enumerate(indices):
        if idx >= nodes[0].shape[0]:
            continue
        node = int(idx)
        for l in range(depth):
            first, k = node - node % arity, 0
            for c in range(arity):
                if c == node % arity:
                    continue
                if first + c < nodes[l].shape[0]:
                    out[t, l, k] = nodes[l][first + c]
                elif pad is not None:
                    out[t, l, k] = pad[l]
                k += 1
            node //= arity
    return out


def small_tree(oracle, arity, n_leaves, padded, seed):
    leaves = edge_scalars(n_leaves, seed)
    depth, n = 0, n_leaves
    while n > 1:
        n = -(-n // arity)
        depth += 1
    pad = edge_scalars(depth, seed + 1).reshape(depth, 4) if padded else None
    return leaves, depth, pad, oracle.merkle_tree(leaves, arity, TAG[arity], 1, pad)


@pytest.mark.parametrize("arity,n_leaves,padded", [(2, 7, False), (3, 20, True), (4, 19, True)])
def test_open(oracle, arity, n_leaves, padded):
    """k_merkle_open (one form: a thread per 16 bytes of path) on an oracle-built tree of depth 3, 300 queries with the ends
    of the tree and two indices outside it: every sibling, pad[l] past the end of a level, zeros for the outsiders."""
    leaves, depth, pad, levels = small_tree(oracle, arity, n_leaves, padded, 70 + arity)
    nq = 300
    idx = np.random.default_rng(72).integers(0, n_leaves, size=nq, dtype=np.uint64)
    idx[:4] = [0, n_leaves - 1, n_leaves, (1 << 64) - 1]
    s = HS.Script("merkle")
    s.buf("leaves", leaves.tobytes())
    s.buf("tree", np.concatenate(levels).tobytes())
    s.buf("idx", idx.tobytes())
    s.fill("paths", nq * depth * (arity - 1) * 32, 0xFF)
    if padded:
        s.buf("pad", pad.tobytes())
        s.call("hades252_merkle_open_pad_dev", "leaves", "tree", n_leaves, arity, "idx", nq, "pad", "paths", None)
    else:
        s.call("hades252_merkle_open_dev", "leaves", "tree", n_leaves, arity, "idx", nq, "paths", None)
    s.dump("paths")
    r = s.run(timeout=300)                               # measured: 1 s
    assert [rc for _, rc in r.rc] == [0]
    exp = expected_paths(leaves, levels, arity, idx, pad)
    assert (u64(r.out["paths"]).reshape(exp.shape) == exp).all()


@pytest.mark.parametrize("arity,n_leaves,padded,form", [(2, 3, False, "coop"), (3, 7, True, "fast"), (4, 13, True, "fast")])
def test_verify_five_waves_and_per_lane(oracle, arity, n_leaves, padded, form):
    """hades252_merkle_verify_dev on the oracle's openings of a depth-2 tree, at the first size of the five-waves form
    (4 097 queries) and of the per-lane form (16 385): every root is the tree's; an index outside the tree with an
    all-zero path gives what the oracle recomputes from it."""
    leaves, depth, pad, levels = small_tree(oracle, arity, n_leaves, padded, 75 + arity)
    assert depth == 2
    nq = FORM_SIZES[form][0]
    assert verify_form(nq, arity) == ("k_merkle_verify_coop<%d>" if form == "coop" else "k_merkle_verify<%d>") % arity
    idx = np.random.default_rng(73).integers(0, n_leaves, size=nq, dtype=np.uint64)
    idx[:4] = [0, n_leaves - 1, n_leaves, (1 << 64) - 1]
    paths = expected_paths(leaves, levels, arity, idx, pad)
    ql = leaves.reshape(-1, 4)[np.minimum(idx, n_leaves - 1).astype(np.int64)]
    s = HS.Script("merkle")
    s.buf("ql", ql.tobytes())
    s.buf("idx", idx.tobytes())
    s.buf("paths", paths.tobytes())
    s.fill("roots", 32 * nq, 0xFF)
    s.call("hades252_merkle_verify_dev", "ql", "idx", "paths", nq, depth, arity, tag_buf(s, arity), 1, "roots", None)
    s.dump("roots")
    r = s.run(timeout=900)                               # measured: 13 s (five waves: 65 blocks x 2 permutations) / 4 s (per lane)
    assert [rc for _, rc in r.rc] == [0]
    roots = u64(r.out["roots"]).reshape(nq, 4)
    assert (roots[idx < n_leaves] == levels[-1]).all()
    for t in (2, 3):
        assert (roots[t] == oracle.merkle_verify_path(leaves.reshape(-1, 4)[n_leaves - 1], int(idx[t]),
                                                      np.zeros((depth, arity - 1, 4), dtype=np.uint64), arity, TAG[arity],
                                                      1)).all()


def test_update_per_lane_levels(oracle, monkeypatch):
    """hades252_merkle_update_dev, arity 4, 65 560 leaves, 16 385 updates: level 1 (16 390 parents, more than the updates)
    runs k_merkle_update_fast, level 2 (4 098 parents from a ragged level, fewer than the updates) is recomputed whole, one
    parent per lane; the DPP forms above are over the block budget and given up."""
    monkeypatch.setenv("HOSTSIM_DPP_MAX_BLOCKS", "0")
    arity, n_leaves, nu = 4, 4 * 16390, FORM_SIZES["fast"][0]
    assert update_form(nu, arity) == "k_merkle_update_fast<4>"
    leaves = edge_scalars(n_leaves, 80)
    old = oracle.merkle_tree(leaves, arity, TAG[arity], 1)
    rng = np.random.default_rng(81)
    idx = np.sort(rng.choice(n_leaves, size=nu, replace=False)).astype(np.uint64)
    idx[-1] = n_leaves + 5                                 # ignored
    new_leaves = leaves.reshape(-1, 4).copy()
    new_leaves[idx[:-1].astype(np.int64)] = edge_scalars(nu - 1, 82).reshape(-1, 4)
    new = oracle.merkle_tree(new_leaves.reshape(-1), arity, TAG[arity], 1)
    s = HS.Script("merkle")
    s.buf("leaves", new_leaves.tobytes())
    s.buf("tree", np.concatenate(old).tobytes())
    s.buf("idx", idx.tobytes())
    s.call("hades252_merkle_update_dev", "leaves", "tree", n_leaves, arity, tag_buf(s, arity), 1, None, "idx", nu, None)
    s.dump("tree")
    r = s.run(timeout=900)                               # measured: 9 s
    assert r.rc == [("hades252_merkle_update_dev", 0)] and "over_budget hades252_merkle_update_dev" in r.stdout
    assert [l.size // 4 for l in new[:3]] == [16390, 4098, 1025]
    tree, off = u64(r.out["tree"]), 0
    for l in range(2):
        assert (tree[off:off + new[l].size] == new[l]).all(), "level %d" % (l + 1)
        off += new[l].size
    assert (tree[off:] == np.concatenate(old[2:])).all()   # the levels of the DPP forms: untouched


def test_update_five_waves_level(oracle, monkeypatch):
    """4 097 updates on the same shape: every level above the updates' count runs k_merkle_update_coop."""
    monkeypatch.setenv("HOSTSIM_DPP_MAX_BLOCKS", "0")
    arity, n_leaves, nu = 4, 4 * 4100, FORM_SIZES["coop"][0]
    assert update_form(nu, arity) == "k_merkle_update_coop<4>"
    leaves = edge_scalars(n_leaves, 83)
    old = oracle.merkle_tree(leaves, arity, TAG[arity], 1)
    idx = np.arange(0, 4 * nu, 4, dtype=np.uint64) + np.uint64(1)          # one leaf under each of 4 097 level-1 parents
    new_leaves = leaves.reshape(-1, 4).copy()
    new_leaves[idx.astype(np.int64)] = edge_scalars(nu, 84).reshape(-1, 4)
    new = oracle.merkle_tree(new_leaves.reshape(-1), arity, TAG[arity], 1)
    s = HS.Script("merkle")
    s.buf("leaves", new_leaves.tobytes())
    s.buf("tree", np.concatenate(old).tobytes())
    s.buf("idx", idx.tobytes())
    s.call("hades252_merkle_update_dev", "leaves", "tree", n_leaves, arity, tag_buf(s, arity), 1, None, "idx", nu, None)
    s.dump("tree")
    r = s.run(timeout=900)                               # measured: 8 s
    assert r.rc == [("hades252_merkle_update_dev", 0)] and "over_budget hades252_merkle_update_dev" in r.stdout
    tree = u64(r.out["tree"])
    assert new[0].size // 4 == 4100
    assert (tree[:new[0].size] == new[0]).all()
    assert (tree[new[0].size:] == np.concatenate(old[1:])).all()


# ---- the DPP forms of hades_lanes.hpp: one parent / query / update per wave (with a helper wave, and without) and per row --
# form: tests/hostsim/hostsim_main.cpp, namespace forms.  The helped form is what the dispatch gives every size used here;
# the unhelped form (769 .. 1 024) and the rows form (1 025 .. 4 096) cost minutes at their own sizes and are launched with
# their call sites' geometry by the form_* launchers.
HELPED, UNHELPED, PER_ROW = 0, 1, 2
assert 5 < FORM_SIZES["lanes"][0] < FORM_SIZES["rows"][0] and FORM_SIZES["lanes_helped"][0] == 1


@pytest.mark.parametrize("form,arity,n_children,padded", [
    (HELPED, 1, 3, False),       # a full block: three parent waves and the helper
    (HELPED, 2, 7, True),        # four parents from a ragged padded level: a second block with idle waves
    (HELPED, 3, 8, True),
    (HELPED, 4, 1, True),        # a lone wave: one child and three copies of the padding digest
    (UNHELPED, 1, 4, False),     # one block of four parent waves
    (UNHELPED, 3, 13, True),     # five parents, ragged and padded: a second block whose other waves return at once
    (PER_ROW, 1, 4, False), (PER_ROW, 2, 9, True), (PER_ROW, 3, 11, False), (PER_ROW, 4, 17, True)])
def test_level_one_parent_per_wave_and_per_row(oracle, form, arity, n_children, padded):
    n_parents = -(-n_children // arity)
    ch = edge_scalars(n_children, 140 + 10 * form + arity)
    pad = edge_scalars(1, 199) if padded else None
    s = HS.Script("merkle")
    s.buf("ch", ch.tobytes())
    s.fill("par", 32 * n_parents, 0xFF)
    if padded:
        s.buf("pad", pad.tobytes())
    if form == HELPED:
        assert level_form(n_children, arity) == "k_merkle_lanes<%d, true>" % arity
        s.call("hades252_merkle_level_pad_dev", "ch", n_children, "par", arity, tag_buf(s, arity), 1, "pad" if padded else None,
               None)
    else:
        s.call("form_merkle_level", arity, "ch", n_children, "par", n_parents, tag_buf(s, arity), 1, "pad" if padded else None,
               form)
    s.dump("par")
    r = s.run(timeout=600)                               # measured: 2 .. 8 s
    assert [rc for _, rc in r.rc] == [0] and "over_budget" not in r.stdout and "not_emulated" not in r.stdout
    assert (u64(r.out["par"]) == oracle.merkle_level_pad(ch, arity, TAG[arity], 1, pad)).all()


@pytest.mark.parametrize("arity,n_leaves,padded", [(4, 13, True), (2, 3, False)])
def test_small_tree_whole_and_root(oracle, arity, n_leaves, padded):
    """merkle_run end to end, nothing given up: hades252_merkle_build[_pad]_dev writes EVERY level of the oracle's tree, and
    hades252_merkle_root[_pad]_dev, ping-ponging through its scratch, the same root."""
    s, leaves, levels, pad, tree_bytes = run_tree(oracle, arity, n_leaves, padded, 160 + arity)
    sizes = [l.size // 4 for l in levels]
    assert sizes[-1] == 1 and len(sizes) == 2
    scratch = 32 * (sizes[0] + sizes[1])
    s.fill("scratch", scratch, 0xFF)
    s.fill("root", 32, 0xFF)
    s.call("hades252_merkle_scratch_bytes", n_leaves, arity)
    if padded:
        s.call("hades252_merkle_root_pad_dev", "leaves", n_leaves, arity, "scratch", scratch, tag_buf(s, arity), 1, "pad", "root",
               None)
    else:
        s.call("hades252_merkle_root_dev", "leaves", n_leaves, arity, "scratch", scratch, tag_buf(s, arity), 1, "root", None)
    s.dump("root")
    r = s.run(timeout=900)                               # measured: 12 .. 18 s
    assert [rc for _, rc in r.rc] == [tree_bytes, 0, scratch, 0]
    assert "over_budget" not in r.stdout and "not_emulated" not in r.stdout
    assert (u64(r.out["tree"]) == np.concatenate(levels)).all()
    assert (u64(r.out["root"]) == levels[-1]).all()


def test_small_tree_merkle4_root_and_empty_digests(oracle):
    """hades252_merkle4_root_dev on 16 leaves (levels of 4 and 1 parents), and hades252_merkle_empty_digests_dev: the table
    pad[l + 1] = the parent of `arity` copies of pad[l], one k_merkle_lanes launch of one parent per level."""
    arity, n_leaves, depth = 4, 16, 3
    leaves = edge_scalars(n_leaves, 170)
    levels = oracle.merkle_tree(leaves, arity, TAG[arity], 1)
    e0 = edge_scalars(1, 171)
    s = HS.Script("merkle")
    s.buf("leaves", leaves.tobytes())
    s.fill("scratch", 32 * 5, 0xFF)
    s.fill("root", 32, 0xFF)
    s.call("hades252_merkle4_root_dev", "leaves", n_leaves, "scratch", 32 * 5, tag_buf(s, arity), 1, "root", None)
    s.buf("e0", e0.tobytes())
    s.fill("pad", 32 * depth, 0xFF)
    s.call("hades252_merkle_empty_digests_dev", 3, depth, "e0", tag_buf(s, 3), 1, "pad", None)
    s.dump("root")
    s.dump("pad")
    r = s.run(timeout=600)                               # measured: 14 s
    assert [rc for _, rc in r.rc] == [0, 0] and "over_budget" not in r.stdout and "not_emulated" not in r.stdout
    assert (u64(r.out["root"]) == levels[-1]).all()
    exp = [e0]
    for l in range(depth - 1):
        exp.append(oracle.merkle_level(np.tile(exp[-1], 3), 3, TAG[3], 1))
    assert (u64(r.out["pad"]) == np.concatenate(exp)).all()


def updated_trees(oracle, arity, n_leaves, idx, seed, pad=None):
    leaves = edge_scalars(n_leaves, seed)
    old = oracle.merkle_tree(leaves, arity, TAG[arity], 1, pad)
    new_leaves = leaves.reshape(-1, 4).copy()
    inside = np.array([i for i in idx if i < n_leaves], dtype=np.int64)
    new_leaves[inside] = edge_scalars(len(inside), seed + 1).reshape(-1, 4)
    return new_leaves, old, oracle.merkle_tree(new_leaves.reshape(-1), arity, TAG[arity], 1, pad)


def test_update_small_tree_whole(oracle):
    """hades252_merkle_update_dev, arity 4, 61 leaves with a padding table, three updates (two under one parent, so one
    update wave stands idle; the fourth index lies outside the tree): levels of 16 and 4 parents run k_merkle_update_lanes,
    the root level is recomputed whole.  The WHOLE tree is the oracle's tree of the new leaves."""
    arity, n_leaves = 4, 61
    idx = np.array([2, 3, 60, n_leaves + 5], dtype=np.uint64)
    pad = edge_scalars(3, 181).reshape(3, 4)
    new_leaves, old, new = updated_trees(oracle, arity, n_leaves, idx, 180, pad)
    assert [l.size // 4 for l in new] == [16, 4, 1] and update_form(len(idx), arity) == "k_merkle_update_lanes<4, true>"
    s = HS.Script("merkle")
    s.buf("leaves", new_leaves.tobytes())
    s.buf("tree", np.concatenate(old).tobytes())
    s.buf("idx", idx.tobytes())
    s.buf("pad", pad.tobytes())
    s.call("hades252_merkle_update_dev", "leaves", "tree", n_leaves, arity, tag_buf(s, arity), 1, "pad", "idx", len(idx), None)
    s.dump("tree")
    r = s.run(timeout=600)                               # measured: 16 s
    assert r.rc == [("hades252_merkle_update_dev", 0)] and "over_budget" not in r.stdout and "not_emulated" not in r.stdout
    assert (u64(r.out["tree"]) == np.concatenate(new)).all()
    assert not (np.concatenate(new) == np.concatenate(old)).all()


@pytest.mark.parametrize("form", [UNHELPED, PER_ROW], ids=["unhelped", "rows"])
def test_update_one_level_unhelped_and_rows(oracle, form):
    """k_merkle_update_lanes<4, false> and k_merkle_update_rows<4> on the first level of a 64-leaf tree: five updates (two
    under one parent, one outside the tree): the parents of the changed leaves are the new tree's, the others untouched."""
    arity, n_leaves = 4, 64
    idx = np.array([0, 1, 37, 63, n_leaves], dtype=np.uint64)
    new_leaves, old, new = updated_trees(oracle, arity, n_leaves, idx, 185 + form)
    s = HS.Script("merkle")
    s.buf("leaves", new_leaves.tobytes())
    s.buf("par", old[0].tobytes())
    s.buf("idx", idx.tobytes())
    s.call("form_merkle_update", arity, "leaves", n_leaves, "par", "idx", len(idx), n_leaves, arity, tag_buf(s, arity), 1, None,
           form)
    s.dump("par")
    r = s.run(timeout=600)                               # measured: 6 s (rows) / 8 s (unhelped)
    assert [rc for _, rc in r.rc] == [0]
    got, exp = u64(r.out["par"]).reshape(-1, 4), old[0].reshape(-1, 4).copy()
    exp[[0, 9, 15]] = new[0].reshape(-1, 4)[[0, 9, 15]]
    assert (got == exp).all() and (got == new[0].reshape(-1, 4)).all() and not (got == old[0].reshape(-1, 4)).all()


@pytest.mark.parametrize("form,arity,n_leaves,padded,nq", [(HELPED, 2, 3, False, 4), (HELPED, 4, 13, True, 1),
                                                           (UNHELPED, 3, 7, True, 4), (PER_ROW, 2, 3, False, 5),
                                                           (PER_ROW, 1, 1, False, 4)])
def test_verify_one_query_per_wave_and_per_row(oracle, form, arity, n_leaves, padded, nq):
    """k_merkle_verify_lanes (helped through the dispatch, unhelped through its launcher) and k_merkle_verify_rows on the
    oracle's openings of a depth-2 tree (arity 1: a chain of two permutations): the first and the last leaf, then random
    ones; every root is the tree's."""
    depth = 2
    if arity == 1:
        leaves, pad = edge_scalars(1, 190), None
        root = oracle.merkle_level(oracle.merkle_level(leaves, 1, TAG[1], 1), 1, TAG[1], 1)
        idx = np.zeros(nq, dtype=np.uint64)
        paths = np.zeros((nq, depth, 0, 4), dtype=np.uint64)
    else:
        leaves, d, pad, levels = small_tree(oracle, arity, n_leaves, padded, 190 + arity)
        assert d == depth
        root = levels[-1]
        idx = np.random.default_rng(191).integers(0, n_leaves, size=nq, dtype=np.uint64)
        idx[:2] = [0, n_leaves - 1][:min(2, nq)]
        paths = expected_paths(leaves, levels, arity, idx, pad)
    ql = leaves.reshape(-1, 4)[idx.astype(np.int64)]
    s = HS.Script("merkle")
    s.buf("ql", ql.tobytes())
    s.buf("idx", idx.tobytes())
    if paths.size:
        s.buf("paths", paths.tobytes())
    s.fill("roots", 32 * nq, 0xFF)
    if form == HELPED:
        assert verify_form(nq, arity) == "k_merkle_verify_lanes<%d, true>" % arity
        s.call("hades252_merkle_verify_dev", "ql", "idx", "paths" if paths.size else None, nq, depth, arity, tag_buf(s, arity), 1,
               "roots", None)
    else:
        s.call("form_merkle_verify", "ql", "idx", "paths" if paths.size else None, nq, depth, arity, tag_buf(s, arity), 1, "roots",
               form)
    s.dump("roots")
    r = s.run(timeout=600)                               # measured: 4 .. 16 s (two dependent permutations per query)
    assert [rc for _, rc in r.rc] == [0]
    assert (u64(r.out["roots"]).reshape(nq, 4) == root).all()
