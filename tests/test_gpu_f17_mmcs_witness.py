"""GPU tier, row f17 (beyond SURVEY section 8): gadget witnesses of mixed-height commitment openings (hades252_wmmcs_inputs /
_witness) against the model (tests/mmcs_witness_model.py), hades252_dmmcs_verify on the same buffers, the fixtures of f14 and
hades252_perm_witness_dev on the inputs.  Exact, byte for byte, everywhere; device outputs sit between sentinel rows."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matrix_model as M  # noqa: E402
import mmcs_model as MM  # noqa: E402
import mmcs_witness_model as WM  # noqa: E402
import witness_chain_model as W  # noqa: E402
import test_wmmcs_abi  # noqa: E402
from gpu_common import CAP, TAG, Guarded, to_dev, to_host  # noqa: E402
from test_gpu_f14_mmcs import _limbs, _p  # noqa: E402

pytestmark = pytest.mark.gpu

INJECT = MM.INJECT
# name -> (arity, heights, cols, pad_mode, out_idx, first generator-B element or None: the fixture's, queries)
SHAPES = {
    "fixture0": MM.GOLDEN_CASES[0][:4] + (1, None, 257),
    "fixture1": MM.GOLDEN_CASES[1][:4] + (1, None, 65),
    "fixture2": MM.GOLDEN_CASES[2][:4] + (1, None, 1),
    "one_group_one_block": (2, (8,), (4,), 0, 1, 23000, 65),       # 4 columns without the pad scalar: exactly one block
    "one_group_pad_block": (2, (8,), (4,), 1, 1, 23000, 257),      # ... and with it a second one that holds the pad alone
    "out_idx_3": (3, (27, 3), (8, 3), 1, 3, 23100, 65),
}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "mmcs_kat.json")) as f:
        return json.load(f)["cases"]


_CASES = {}


def _shape(oracle, name):
    """The openings of a shape, computed once: n queries that walk over every leaf, and the model's chains."""
    if name not in _CASES:
        arity, heights, cols, pad_mode, out_idx, first, n = SHAPES[name]
        if first is None:
            first = MM.GOLDEN_CASES[int(name[-1])][5]
        groups = MM.golden_groups(oracle, heights, cols, first)
        tree, root = MM.commit(oracle, groups, arity, pad_mode=pad_mode, out_idx=out_idx)
        idx = [(5 * t + 1) % heights[0] for t in range(n)]
        assert n < heights[0] or set(idx) == set(range(heights[0]))
        paths = MM.open_paths(tree, heights[0], arity, idx)
        rows = [MM.open_rows(groups, i) for i in idx]
        ins, outs = WM.batch(oracle, rows, heights, idx, paths, arity, pad_mode=pad_mode, out_idx=out_idx)
        assert all(outs[-1, q, out_idx].tobytes() == root.tobytes() for q in range(n))
        _CASES[name] = dict(arity=arity, heights=heights, cols=cols, pad_mode=pad_mode, out_idx=out_idx, n=n, groups=groups, root=root,
                            idx=idx, paths=paths, rows=np.stack([MM.flat_rows(r) for r in rows]), inputs=ins, outputs=outs,
                            P=len(WM.steps(heights, cols, arity, pad_mode)))
    return _CASES[name]


class _Dev:
    """The openings of a batch in device memory, and the calls on them through the C ABI."""

    def __init__(self, torch, lib, c, rows=None, idx=None, paths=None):
        self.torch, self.lib, self.c = torch, lib, c
        self.rows = to_dev(torch, c["rows"] if rows is None else rows)
        self.idx = to_dev(torch, np.array(c["idx"] if idx is None else idx, dtype=np.uint64))
        self.paths = to_dev(torch, c["paths"] if paths is None else paths)
        self.n = int(self.idx.numel())
        self.hs, self.cs = np.array(c["heights"], dtype=np.uint64), np.array(c["cols"], dtype=np.uint64)

    def _front(self):
        c = self.c
        return (self.rows.data_ptr(), _p(self.hs), _p(self.cs), len(c["heights"]), self.idx.data_ptr(), self.paths.data_ptr(), self.n,
                c["arity"], _limbs(CAP), c["pad_mode"], _limbs(TAG[c["arity"]]), _limbs(INJECT), c["out_idx"])

    def verify(self):
        roots = Guarded(self.torch, (self.n, 4))
        assert self.lib.hades252_dmmcs_verify(*self._front(), roots.ptr, None) == 0
        return roots.check("verify")

    def inputs(self, want_roots=True, stream=None):
        inputs, roots = Guarded(self.torch, (self.c["P"], self.n, 5, 4)), Guarded(self.torch, (self.n, 4))
        assert self.lib.hades252_wmmcs_inputs(*self._front(), inputs.ptr, roots.ptr if want_roots else None, stream) == 0
        return inputs.check("inputs"), roots.check("roots", interior=want_roots)

    def witness(self, want_roots=True, stream=None):
        inputs, roots = Guarded(self.torch, (self.c["P"], self.n, 5, 4)), Guarded(self.torch, (self.n, 4))
        wires = Guarded(self.torch, (W.WIRES, self.c["P"], self.n, 4))
        rc = self.lib.hades252_wmmcs_witness(*self._front(), inputs.ptr, wires.ptr, roots.ptr if want_roots else None, stream)
        assert rc == 0
        return wires.check("wires"), inputs.check("inputs"), roots.check("roots", interior=want_roots)


def _outputs_of(wires):
    """r2[0 .. 4] of every record, read off the wires: [5, P, n, 4] on the host."""
    return to_host(wires[W.LAST_ROW:W.LAST_ROW + 10:2].contiguous()).reshape(5, *wires.shape[1:])


# ---- 1. inputs, roots and wires of every shape -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_inputs_roots_and_wires_of_every_shape(hades_lib, H, torch_cuda, oracle, golden, name):
    torch, c = torch_cuda, _shape(oracle, name)
    d = _Dev(torch, hades_lib, c)
    n, P, out_idx = c["n"], c["P"], c["out_idx"]
    assert P == H.mmcs_perms(c["heights"], c["cols"], c["arity"], c["pad_mode"]) == hades_lib.hades252_wmmcs_perms(
        _p(d.hs), _p(d.cs), len(c["heights"]), c["arity"], c["pad_mode"])
    wires, inputs, roots = d.witness()
    # the inputs are the model's, the roots those of the fused verification on the same buffers and the committed root
    assert to_host(inputs).tobytes() == c["inputs"].tobytes()
    assert torch.equal(roots, d.verify()) and to_host(roots).tobytes() == np.tile(c["root"], n).tobytes()
    if name.startswith("fixture"):
        assert c["root"].tobytes() == MM.unhex([golden[int(name[-1])]["root"]]).tobytes()
    # the inputs stage alone writes the same inputs and roots
    alone, alone_roots = d.inputs()
    assert torch.equal(alone, inputs) and torch.equal(alone_roots, roots)
    # the defining property, and the root in the last record
    assert torch.equal(wires.view(W.WIRES, P * n, 4), H.perm_witness(inputs.view(P * n, 20)))
    assert torch.equal(wires[W.LAST_ROW + 2 * out_idx, P - 1], roots)
    # the outputs read off the wires are the model's, and every link of the model holds on them
    outs = _outputs_of(wires)
    assert outs.transpose(1, 2, 0, 3).tobytes() == c["outputs"].tobytes()
    inputs_h = to_host(inputs).reshape(P, n, 5, 4)
    linked = 0
    for q, index in enumerate(c["idx"]):
        for t, w, src, sw in WM.links(c["heights"], c["cols"], index, c["arity"], c["pad_mode"], out_idx):
            assert inputs_h[t, q, w].tobytes() == outs[sw, src, q].tobytes(), (q, t, w, src, sw)
            linked += 1
    depth = MM.depth_of(c["heights"][0], c["arity"])
    assert linked >= n * (depth + 2 * (len(c["cols"]) - 1))


# ---- 2. tampered openings ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1, 2])
def test_every_tamper_moves_the_root_and_the_first_affected_input_only(hades_lib, torch_cuda, oracle, golden, case):
    arity, heights, cols, pad_mode, index, first = MM.GOLDEN_CASES[case]
    c = dict(_shape(oracle, "fixture%d" % case))
    groups, depth = c["groups"], MM.depth_of(heights[0], arity)
    tree, root = MM.commit(oracle, groups, arity, pad_mode=pad_mode)
    rows, path = MM.open_rows(groups, index), MM.open_paths(tree, heights[0], arity, [index])[0]
    bad = MM.tampers(rows, index, path, heights[0])
    batch = [("honest", rows, index, path)] + bad
    d = _Dev(torch_cuda, hades_lib, c, rows=np.stack([MM.flat_rows(r) for _, r, _, _ in batch]), idx=[i for _, _, i, _ in batch],
             paths=np.stack([np.asarray(p).reshape(depth, arity - 1, 4) for _, _, _, p in batch]))
    inputs, roots = d.inputs()
    inputs_h, roots_h = to_host(inputs).reshape(c["P"], len(batch), 5, 4), to_host(roots).reshape(-1, 4)
    assert to_host(d.verify()).tobytes() == roots_h.tobytes()
    assert roots_h[0].tobytes() == root.tobytes() == MM.unhex([golden[case]["root"]]).tobytes()
    table = WM.steps(heights, cols, arity, pad_mode)
    for q, (what, r, i, p) in enumerate(batch):
        want, _ = WM.chain(oracle, r, heights, i, p, arity, pad_mode=pad_mode)
        assert inputs_h[:, q].tobytes() == want.tobytes(), what
        if q == 0:
            continue
        assert roots_h[q].tobytes() == MM.unhex([golden[case]["tampered"][q - 1]["root"]]).tobytes() != root.tobytes(), what
        differs = [t for t in range(c["P"]) if inputs_h[t, q].tobytes() != inputs_h[t, 0].tobytes()]
        assert differs and differs[0] == WM.first_affected(table, what, cols, depth), (what, differs)


# ---- 3. no roots, a side stream ------------------------------------------------------------------------------------------
def test_without_roots_on_a_side_stream(hades_lib, H, torch_cuda, oracle):
    torch, c = torch_cuda, _shape(oracle, "fixture1")
    d = _Dev(torch, hades_lib, c)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        inputs, roots = d.inputs(want_roots=False, stream=s.cuda_stream)         # (check() synchronises the device)
        assert to_host(inputs).tobytes() == c["inputs"].tobytes()
        assert bool((roots == -1).all())                                         # d_roots = NULL: nothing was written there
        wires, inputs2, _ = d.witness(want_roots=False, stream=s.cuda_stream)
        assert torch.equal(inputs2, inputs)
        # through Python on the current (side) stream: nothing goes to the default stream
        wires_t, inputs_t, roots_t = H.mmcs_witness_dev(d.rows.view(c["n"], -1, 4), c["heights"], c["cols"], d.idx,
                                                        d.paths.view(c["n"], -1, c["arity"] - 1, 4), c["arity"], CAP, TAG[c["arity"]],
                                                        INJECT, c["pad_mode"], c["out_idx"])
        assert torch.cuda.default_stream().query()
        s.synchronize()
        assert tuple(wires_t.shape) == (W.WIRES, c["P"], c["n"], 4) and tuple(inputs_t.shape) == (c["P"], c["n"], 5, 4)
        assert torch.equal(wires_t, wires) and torch.equal(inputs_t, inputs) and to_host(roots_t).tobytes() == np.tile(c["root"], c["n"]).tobytes()
        inputs_p, roots_p = H.mmcs_inputs_dev(d.rows.view(c["n"], -1, 4), c["heights"], c["cols"], d.idx,
                                              d.paths.view(c["n"], -1, c["arity"] - 1, 4), c["arity"], CAP, TAG[c["arity"]], INJECT,
                                              c["pad_mode"], c["out_idx"])
        s.synchronize()
        assert torch.equal(inputs_p, inputs) and torch.equal(roots_p, roots_t)


# ---- 4. end to end: absorb, commit, open, witness, all on the device -------------------------------------------------------
def test_end_to_end_from_a_row_major_and_a_column_major_group(H, torch_cuda, oracle):
    torch = torch_cuda
    arity, heights, cols = 2, (16, 4), (5, 3)
    groups = MM.golden_groups(oracle, heights, cols, 23500)
    want_tree, want_root = MM.commit(oracle, groups, arity)
    idx = np.array([(7 * t + 3) % 16 for t in range(65)], dtype=np.uint64)
    parts = [to_dev(torch, groups[0]).view(groups[0].shape), to_dev(torch, M.planes_of(groups[1])).view(cols[1], heights[1], 4)]
    layouts = [H._lib.LAYOUT_ROWS, H._lib.LAYOUT_COLS]
    d_idx = to_dev(torch, idx)
    with H.Mmcs(CAP) as mc:
        mc.absorb_dev(parts, layouts)
        torch.cuda.synchronize()                                                 # before the host-form commit
        tree, root = mc.commit(arity, TAG[arity], INJECT)
        assert root.tobytes() == want_root.tobytes()
        rows_t, paths_t = mc.open_dev(parts, d_idx, layouts)
        wires, inputs, roots = H.mmcs_witness_dev(rows_t, heights, cols, d_idx, paths_t, arity, CAP, TAG[arity], INJECT)
        torch.cuda.synchronize()
    P = H.mmcs_perms(heights, cols, arity)
    assert P == 2 + 1 + 4 + 1 and tuple(wires.shape) == (W.WIRES, P, 65, 4) and tuple(inputs.shape) == (P, 65, 5, 4)
    assert to_host(roots).tobytes() == np.tile(want_root, 65).tobytes()
    assert torch.equal(wires.view(W.WIRES, P * 65, 4), H.perm_witness(inputs.view(P * 65, 20)))
    assert torch.equal(wires[W.LAST_ROW + 2, P - 1], roots)
    rows = [MM.open_rows(groups, int(i)) for i in idx]
    want, _ = WM.batch(oracle, rows, heights, idx.tolist(), MM.open_paths(want_tree, 16, arity, idx.tolist()), arity)
    assert to_host(inputs).tobytes() == want.tobytes()
    steps = H.mmcs_steps(heights, cols, arity)
    assert [tuple(int(v) for v in s) for s in steps] == WM.steps(heights, cols, arity, 1)


# ---- 5. the rules, with a device in reach ----------------------------------------------------------------------------------
def test_python_wrappers_refuse_wrong_shapes(H, torch_cuda, monkeypatch):
    test_wmmcs_abi.wrappers_refuse_wrong_shapes(torch_cuda, H, monkeypatch)


def test_nothing_to_do_and_refusals_touch_no_buffer(hades_lib, torch_cuda, oracle):
    torch, c = torch_cuda, _shape(oracle, "fixture2")
    d = _Dev(torch, hades_lib, c)
    inputs, roots = Guarded(torch, (c["P"], 1, 5, 4)), Guarded(torch, (1, 4))
    front = list(d._front())
    assert hades_lib.hades252_wmmcs_inputs(*front[:6], 0, *front[7:], inputs.ptr, roots.ptr, None) == 0      # n_queries = 0
    assert hades_lib.hades252_wmmcs_inputs(*front, inputs.ptr + 8, roots.ptr, None) == -1                    # misaligned inputs
    assert hades_lib.hades252_wmmcs_witness(*front, inputs.ptr, None, roots.ptr, None) == -1                 # no wires
    front[12] = 5
    assert hades_lib.hades252_wmmcs_inputs(*front, inputs.ptr, roots.ptr, None) == -1                        # out_idx
    inputs.check("refused", interior=False)
    roots.check("refused", interior=False)
    assert bool((inputs.t == -1).all()) and bool((roots.t == -1).all())
