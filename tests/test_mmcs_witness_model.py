"""CPU tier: the model of the mixed-height commitment witness (tests/mmcs_witness_model.py) against what it is defined
through -- the step count and the root of tests/mmcs_model.py for the three fixture shapes and every tampered opening, the
links between the records (every inject and climb input is the output the header names), the sponge's first block and add
gates, and a hand-written step table."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mmcs_model as MM  # noqa: E402
import mmcs_witness_model as WM  # noqa: E402
import oracle_lib  # noqa: E402
from gpu_common import CAP, TAG  # noqa: E402

S_, I_, C_ = WM.SPONGE, WM.INJECT, WM.CLIMB


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "mmcs_kat.json")) as f:
        return json.load(f)["cases"]


def _openings(oracle, case):
    """The fixture's opening and its tampers: [(label, rows, index, path)]."""
    arity, heights, cols, pad_mode, index, first = MM.GOLDEN_CASES[case]
    groups = MM.golden_groups(oracle, heights, cols, first)
    tree, _ = MM.commit(oracle, groups, arity, pad_mode=pad_mode)
    rows, path = MM.open_rows(groups, index), MM.open_paths(tree, heights[0], arity, [index])[0]
    return [("honest", rows, index, path)] + MM.tampers(rows, index, path, heights[0])


def test_the_step_table_of_the_first_fixture_shape_by_hand():
    # heights 8 / 4 / 1 at arity 2 (levels 3 / 2 / 0), 5 / 3 / 2 columns under pad_mode 1: 2 + 1 + 1 blocks
    assert WM.steps((8, 4, 1), (5, 3, 2), 2, 1) == [(S_, 0, 0), (S_, 0, 1), (C_, 0, 0), (S_, 1, 0), (I_, 1, 0), (C_, 1, 1), (C_, 1, 2),
                                                    (S_, 2, 0), (I_, 2, 0)]
    # ... and without the pad scalar the tallest row is still two blocks (5 columns), the others one
    assert WM.steps((8, 4, 1), (5, 3, 2), 2, 0) == WM.steps((8, 4, 1), (5, 3, 2), 2, 1)
    assert WM.steps((16, 4), (4, 1), 4, 0) == [(S_, 0, 0), (C_, 0, 0), (S_, 1, 0), (I_, 1, 0), (C_, 1, 1)]
    assert WM.steps((16, 4), (4, 1), 4, 1)[:3] == [(S_, 0, 0), (S_, 0, 1), (C_, 0, 0)]
    assert WM.steps((8,), (4,), 2, 0) == [(S_, 0, 0), (C_, 0, 0), (C_, 0, 1), (C_, 0, 2)]
    assert (WM.SPONGE, WM.INJECT, WM.CLIMB) == (0, 1, 2)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_count_root_and_links_for_the_fixture_and_every_tamper(oracle, golden, case):
    arity, heights, cols, pad_mode, _, _ = MM.GOLDEN_CASES[case]
    depth = MM.depth_of(heights[0], arity)
    table = WM.steps(heights, cols, arity, pad_mode)
    assert len(table) == MM.permutations(cols, depth, pad_mode)
    assert [s for s in table if s[0] == C_] == [(C_, g, l) for l, g in enumerate(s[1] for s in table if s[0] == C_)]
    assert sum(s[0] == C_ for s in table) == depth and sum(s[0] == I_ for s in table) == len(cols) - 1
    want_roots = [golden[case]["root"]] + [t["root"] for t in golden[case]["tampered"]]
    for (what, rows, index, path), want in zip(_openings(oracle, case), want_roots):
        ins, outs = WM.chain(oracle, rows, heights, index, path, arity, pad_mode=pad_mode)
        assert ins.shape == outs.shape == (len(table), 5, 4), what
        assert outs.tobytes() == oracle.perm_batch(ins.reshape(-1)).tobytes(), what
        root = MM.verify(oracle, rows, heights, index, path, arity, pad_mode=pad_mode)
        assert outs[-1, 1].tobytes() == root.tobytes() == MM.unhex([want]).tobytes(), what
        # every inject and climb input is linked to the outputs the header names (and a later block keeps word 0)
        linked = WM.links(heights, cols, index, arity, pad_mode)
        for t, w, src, sw in linked:
            assert 0 <= src < t and ins[t, w].tobytes() == outs[src, sw].tobytes(), (what, t, w, src, sw)
        assert sum(table[t][0] == I_ for t, _, _, _ in linked) == 2 * (len(cols) - 1)
        assert sum(table[t][0] == C_ for t, _, _, _ in linked) == depth
        # what is not linked is data: tags, capacity, siblings, zeros, and the blocks added into words 1..4
        path = np.asarray(path).reshape(depth, arity - 1, 4)
        for t, (kind, g, o) in enumerate(table):
            if kind == S_:
                row = [oracle_lib.int_of(w) for w in rows[g]] + ([WM.ONE] if pad_mode == 1 else [])
                block = (row + [0] * 8)[4 * o:4 * o + 4]
                before = [0] * 5 if o == 0 else [oracle_lib.int_of(w) for w in outs[t - 1]]
                assert [oracle_lib.int_of(w) for w in ins[t, 1:]] == [(a + b) % WM.P for a, b in zip(before[1:], block)], (what, t)
                if o == 0:
                    assert oracle_lib.int_of(ins[t, 0]) == CAP
            elif kind == I_:
                assert oracle_lib.int_of(ins[t, 0]) == MM.INJECT and not ins[t, 3:].any()
            else:
                pos = (index // arity ** o) % arity
                assert oracle_lib.int_of(ins[t, 0]) == TAG[arity] and not ins[t, 1 + arity:].any()
                assert np.delete(ins[t, 1:1 + arity], pos, axis=0).tobytes() == path[o].tobytes(), (what, t)


def test_a_tamper_changes_the_first_affected_input_and_nothing_before_it(oracle):
    for case in range(3):
        arity, heights, cols, pad_mode, _, _ = MM.GOLDEN_CASES[case]
        table = WM.steps(heights, cols, arity, pad_mode)
        (_, rows, index, path), *bad = _openings(oracle, case)
        honest, _ = WM.chain(oracle, rows, heights, index, path, arity, pad_mode=pad_mode)
        for what, r, i, p in bad:
            ins, _ = WM.chain(oracle, r, heights, i, p, arity, pad_mode=pad_mode)
            first = WM.first_affected(table, what, cols, MM.depth_of(heights[0], arity))
            differs = [t for t in range(len(table)) if ins[t].tobytes() != honest[t].tobytes()]
            assert differs and differs[0] == first, (case, what, differs, first)
