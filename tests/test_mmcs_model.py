"""CPU tier: the model of the mixed-height matrix commitments (tests/mmcs_model.py) against what it is defined through -- the
one-matrix commitment of tests/matrix_model.py, the oracle's Merkle level at arity 2 for the injection -- its own round trip
(open, then verify, for every index), its tampered roots, and the committed fixture tests/golden/mmcs_kat.json."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matrix_model as M  # noqa: E402
import mmcs_model as MM  # noqa: E402
from gpu_common import CAP, TAG  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "mmcs_kat.json")) as f:
        return json.load(f)["cases"]


def test_the_fixture_is_the_models_and_has_the_three_shapes(oracle, golden):
    assert [(c["arity"], c["heights"], c["cols"], c["pad_mode"]) for c in golden] == \
        [(2, [8, 4, 1], [5, 3, 2], 1), (4, [16, 4], [4, 1], 0), (3, [9, 1], [1, 6], 1)]
    with open(os.path.join(ROOT, "tests", "golden", "mmcs_kat.json")) as f:
        assert f.read() == json.dumps(MM.golden(oracle), indent=1) + "\n", "stale: python tools/gen_mmcs_kat.py"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mmcs_kat.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "current", r.stdout + r.stderr


@pytest.mark.parametrize("arity", [2, 3, 4])
@pytest.mark.parametrize("pad_mode", [0, 1])
def test_one_group_is_the_one_matrix_commitment(oracle, arity, pad_mode):
    n_rows = arity ** 2
    m = oracle.gen_b(19500, n_rows * 5).reshape(n_rows, 5, 4)
    digests, tree, root = M.commit(oracle, m, arity, pad_mode=pad_mode)
    got_tree, got_root = MM.commit(oracle, [m], arity, pad_mode=pad_mode)
    assert got_tree.tobytes() == np.concatenate([digests, tree]).tobytes() and got_root.tobytes() == root.tobytes()
    assert got_tree.shape[0] == MM.tree_nodes(n_rows, arity)
    # ... and so are its openings and their verification
    idx = list(range(n_rows)) + [n_rows, n_rows + 7]
    rows, paths = M.open_rows(m, digests, tree, arity, idx)
    assert MM.open_paths(got_tree, n_rows, arity, idx).tobytes() == paths.tobytes()
    assert not paths[n_rows:].any()
    for i in (0, n_rows - 1):
        assert MM.verify(oracle, [m[i]], [n_rows], i, paths[i], arity, pad_mode=pad_mode).tobytes() == \
            M.verify(oracle, m[i], i, paths[i], arity, pad_mode=pad_mode).tobytes() == root.tobytes()


def test_the_injection_is_the_level_at_arity_two_on_the_pair(oracle):
    nodes, leaves = oracle.gen_b(19600, 4).reshape(4, 4), oracle.gen_b(19700, 4).reshape(4, 4)
    got = MM.inject(oracle, nodes, leaves)
    for i in range(4):
        assert got[i].tobytes() == oracle.merkle_level(np.concatenate([nodes[i], leaves[i]]), 2, MM.INJECT).tobytes()
    # by hand on the second fixture shape: one level, the injection of the four-row group, the last level
    tall, short = MM.golden_groups(oracle, (16, 4), (4, 1), 19100)
    tree, root = MM.commit(oracle, [short, tall], 4, pad_mode=0)               # the order of the groups does not matter
    leaf0, leaf1 = M.row_digests(oracle, tall, CAP, 0), M.row_digests(oracle, short, CAP, 0)
    level1 = MM.inject(oracle, oracle.merkle_level(leaf0.reshape(-1), 4, TAG[4]).reshape(-1, 4), leaf1)
    assert tree.tobytes() == np.concatenate([leaf0, level1, oracle.merkle_level(level1.reshape(-1), 4, TAG[4]).reshape(-1, 4)]).tobytes()
    assert root.tobytes() == tree[-1].tobytes()


def test_open_then_verify_round_trips_for_every_index_and_every_tamper_moves_the_root(oracle, golden):
    for c, (arity, heights, cols, pad_mode, index, first) in zip(golden, MM.GOLDEN_CASES):
        groups = MM.golden_groups(oracle, heights, cols, first)
        for g, hexes in zip(groups, c["matrices_row_major"]):
            assert MM.unhex(hexes).tobytes() == g.tobytes()
        tree, root = MM.unhex(c["tree"]), MM.unhex([c["root"]])[0]
        assert tree.shape[0] == MM.tree_nodes(heights[0], arity) and tree[-1].tobytes() == root.tobytes()
        assert MM.commit(oracle, groups, arity, pad_mode=pad_mode)[0].tobytes() == tree.tobytes()
        paths = MM.open_paths(tree, heights[0], arity, list(range(heights[0] + 1)))
        assert not paths[heights[0]].any()
        for i in range(heights[0]):
            rows = MM.open_rows(groups, i)
            assert [r.shape[0] for r in rows] == list(cols)
            assert MM.verify(oracle, rows, heights, i, paths[i], arity, pad_mode=pad_mode).tobytes() == root.tobytes(), i
        rows, path = MM.open_rows(groups, index), paths[index]
        assert c["opening"]["index"] == index and MM.unhex(c["opening"]["path"]).tobytes() == path.tobytes()
        assert [MM.unhex(r).tobytes() for r in c["opening"]["rows"]] == [r.tobytes() for r in rows]
        bad = MM.tampers(rows, index, path, heights[0])
        assert [t["what"] for t in c["tampered"]] == [b[0] for b in bad] == ["row %d" % g for g in range(len(cols))] + ["sibling", "index"]
        seen = {root.tobytes()}
        for t, (what, r, i, p) in zip(c["tampered"], bad):
            got = MM.verify(oracle, r, heights, i, p, arity, pad_mode=pad_mode)
            assert got.tobytes() == MM.unhex([t["root"]]).tobytes(), what
            assert got.tobytes() not in seen, what                          # each tamper moves the root, each elsewhere
            seen.add(got.tobytes())


def test_the_permutation_count():
    # the measured shape of tools/time_mmcs.py: heights 2^20 / 2^16, columns 8 / 4, pad_mode 1 -> 3 + 2 blocks, 20 levels, one injection
    assert MM.permutations((8, 4), 20, 1) == 26
    assert MM.permutations((5, 3, 2), 3, 1) == 2 + 1 + 1 + 3 + 2 and MM.permutations((4, 1), 2, 0) == 1 + 1 + 2 + 1
