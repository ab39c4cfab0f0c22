"""Hades252 run backwards (TEST INFRASTRUCTURE ONLY): the input whose state at a chosen stage of a chosen round is a chosen
target, and a catalogue of such inputs that puts edge values INSIDE the rounds -- where the kernels hold lazily reduced,
scaled values and their exit and reduction routines take their rare branches.

Every round is invertible: x -> x^5 is a bijection of the field (gcd(5, p - 1) = 1, inverse x -> x^D with D = 5^-1 mod
p - 1), the Cauchy MDS matrix is invertible mod p and the round key is an addition.  Pure Python big integers over
oracle/hades_spec.py; the stages of round r, in the spec's order (src/strategies.rs:79-119):

    "sbox_in"   after the round key, before the S-boxes
    "mds_in"    after the S-boxes (all words in a full round, word 4 in a partial one), before the matrix
    "out"       after the matrix: trace[r] of hades_spec.perm
"""
from __future__ import annotations

import functools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hades_spec as S  # noqa: E402
from hades252_amd import _derive as D  # noqa: E402

P = S.P
WIDTH = S.WIDTH
ROUNDS = S.TOTAL_FULL_ROUNDS + S.PARTIAL_ROUNDS
STAGES = ("sbox_in", "mds_in", "out")
SBOX_INV = pow(5, -1, P - 1)                     # x -> x^SBOX_INV undoes x -> x^5


def is_full(r: int) -> bool:
    return D.is_full_round(r)


@functools.lru_cache(maxsize=None)
def mds_inverse() -> tuple:
    """M^-1 mod p by Gauss-Jordan elimination, checked against hades_spec.mds_matrix()."""
    m = S.mds_matrix()
    a = [list(row) + [int(i == j) for j in range(WIDTH)] for i, row in enumerate(m)]
    for c in range(WIDTH):
        piv = next(i for i in range(c, WIDTH) if a[i][c])
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], -1, P)
        a[c] = [v * inv % P for v in a[c]]
        for i in range(WIDTH):
            if i != c and a[i][c]:
                f = a[i][c]
                a[i] = [(v - f * w) % P for v, w in zip(a[i], a[c])]
    minv = tuple(tuple(row[WIDTH:]) for row in a)
    for i in range(WIDTH):
        for j in range(WIDTH):
            assert sum(m[i][k] * minv[k][j] for k in range(WIDTH)) % P == int(i == j)
    return minv


def _matvec(m, v):
    return [sum(m[i][j] * v[j] for j in range(WIDTH)) % P for i in range(WIDTH)]


def _ark(r: int) -> list:
    return S.round_constants()[WIDTH * r: WIDTH * r + WIDTH]


def round_fwd(state, r: int) -> list:
    """Round r of hades_spec.perm on one state."""
    st = [(v + c) % P for v, c in zip(state, _ark(r))]
    st = [S.quintic_s_box(v) for v in st] if is_full(r) else st[:4] + [S.quintic_s_box(st[4])]
    return _matvec(S.mds_matrix(), st)


def _back(state, r: int, stage: str) -> list:
    """The state entering round r (trace[r - 1], or the input for r = 0) whose `stage` of round r is `state`."""
    st = list(state)
    if stage == "out":
        st = _matvec(mds_inverse(), st)
    if stage in ("out", "mds_in"):
        st = [pow(v, SBOX_INV, P) for v in st] if is_full(r) else st[:4] + [pow(st[4], SBOX_INV, P)]
    return [(v - c) % P for v, c in zip(st, _ark(r))]


def unround(state, r: int) -> list:
    """The inverse of round r: unround(round_fwd(x, r), r) == x."""
    return _back(state, r, "out")


def input_for(r: int, stage: str, target) -> list:
    """The canonical input whose state at `stage` of round `r` equals `target` (five field values in [0, p))."""
    assert stage in STAGES and 0 <= r < ROUNDS and len(target) == WIDTH and all(0 <= v < P for v in target)
    st = _back(target, r, stage)
    for rr in range(r - 1, -1, -1):
        st = unround(st, rr)
    return st


def stages_of(inp) -> list:
    """[{stage: five values}] for every round of hades_spec's schedule, computed forward from `inp`."""
    out, st = [], list(inp)
    for r in range(ROUNDS):
        a = [(v + c) % P for v, c in zip(st, _ark(r))]
        b = [S.quintic_s_box(v) for v in a] if is_full(r) else a[:4] + [S.quintic_s_box(a[4])]
        st = _matvec(S.mds_matrix(), b)
        out.append({"sbox_in": a, "mds_in": b, "out": st})
    return out


@functools.lru_cache(maxsize=None)
def gadget_layout() -> tuple:
    """Wire indices of hades_spec.perm_gadget's 972 gate outputs, per round r: {"sbox_in": five wires whose values are the
    state at "sbox_in" (round 0's key additions, else the previous round's r2 rows), "sbox": {word: (v2, v4, v5)},
    "r1": five, "r2": five}."""
    lay, g, prev_r2 = [], 5, list(range(5))
    for r in range(ROUNDS):
        sb = {}
        for w in (range(WIDTH) if is_full(r) else (WIDTH - 1,)):
            sb[w] = (g, g + 1, g + 2)
            g += 3
        r1 = [g + 2 * j for j in range(WIDTH)]
        r2 = [g + 2 * j + 1 for j in range(WIDTH)]
        g += 2 * WIDTH
        lay.append({"sbox_in": prev_r2, "sbox": sb, "r1": r1, "r2": r2})
        prev_r2 = r2
    assert g == D.WITNESS_WIRES
    return tuple(lay)


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------
class Label(tuple):
    """(round, stage, words, values, kind): the state at `stage` of round `round` holds values[i] in word words[i] (field
    values); `kind` says why: "edge" / "sbox_edge" (an edge value), "zero" (a true zero), "held_zero" (the value the
    scale-tracked kernels hold as zero), "r1_zero" (a zero r1 gadget wire)."""

    def __new__(cls, r, stage, words, values, kind):
        return super().__new__(cls, (r, stage, tuple(words), tuple(values), kind))

    r = property(lambda s: s[0])
    stage = property(lambda s: s[1])
    words = property(lambda s: s[2])
    values = property(lambda s: s[3])
    kind = property(lambda s: s[4])

    def __str__(self):
        vals = ",".join(VALUE_NAMES.get(v, "%#x" % v) for v in self.values)
        return "r%d/%s/w%s=%s/%s" % (self.r, self.stage, "".join(map(str, self.words)), vals, self.kind)


M1 = S.from_mont(1)                   # the value stored as the in-memory word 1
MP1 = S.from_mont(P - 1)              # ... as the in-memory word p - 1
M255 = S.from_mont((1 << 255) % P)    # ... as 2^255 mod p
VALUE_NAMES = {0: "0", 1: "1", P - 1: "-1", M1: "mem(1)", MP1: "mem(p-1)", M255: "mem(2^255)"}

# the rounds whose stages the catalogue reaches: the first full rounds, the first partial rounds, one in the middle, the
# last partial rounds (the hand-over of the deferred constants) and the trailing full rounds
CATALOGUE_ROUNDS = (0, 1, 3, 4, 5, 33, 61, 62, 63, 64, 65, 66)
SBOX_EDGES = (0, 1, P - 1, M1, MP1)
# the last round's outputs, all five words: values 0, 1, -1 and the in-memory words 1, p - 1, p - R (= value -1), 2^255
OUTPUT_EDGES = (0, 1, P - 1, M1, MP1, S.from_mont(P - S.R), M255)


def held_offsets():
    """(trace_d, pre_d) of the scale-tracked schedule (_derive.effective_constants): true minus held, after round r and
    between the round key and the matrix of round r (words 0..3).  A true value equal to the offset is a HELD zero."""
    _, trace_d = D.effective_constants()
    return trace_d, D._EFF_EXTRA["pre_d"]


@functools.lru_cache(maxsize=None)
def edge_catalogue() -> tuple:
    """Deterministic ((input state, Label), ...), about 12 ms of big-integer work per entry; the words a label leaves free
    are random.  tests/test_round_inverse.py checks that every entry reaches its labelled target in hades_spec."""
    rng = random.Random(0x5EED252)
    trace_d, pre_d = held_offsets()
    mds = S.mds_matrix()
    specs = []

    def add(r, stage, words, values, kind):
        specs.append(Label(r, stage, words, values, kind))

    for v in OUTPUT_EDGES:
        add(ROUNDS - 1, "out", range(WIDTH), [v] * WIDTH, "edge")
    for w in range(WIDTH):
        add(ROUNDS - 1, "out", [w], [0], "zero")
    for r in CATALOGUE_ROUNDS:
        for v in SBOX_EDGES:
            add(r, "sbox_in", [WIDTH - 1], [v], "sbox_edge")
            if is_full(r):
                add(r, "sbox_in", range(WIDTH), [v] * WIDTH, "sbox_edge")
        for w in range(WIDTH):
            add(r, "out", [w], [0], "zero")
        for w in range(WIDTH):
            add(r, "out", [w], [trace_d[r][w]], "held_zero")
        for w in range(WIDTH - 1):
            add(r, "mds_in", [w], [pre_d[r][w]], "held_zero")
        for j in (0, WIDTH - 1):
            add(r, "mds_in", [0, 1, 2], [j, j, j], "r1_zero")        # values filled in below: row j's r1 = 0
    out, seen = [], set()
    for lab in specs:
        tgt = [rng.randrange(P) for _ in range(WIDTH)]
        if lab.kind == "r1_zero":
            j = lab.values[0]                                       # M[j][0] z0 + M[j][1] z1 + M[j][2] z2 = 0
            tgt[0] = -(mds[j][1] * tgt[1] + mds[j][2] * tgt[2]) * pow(mds[j][0], -1, P) % P
            key = (lab.r, lab.stage, "r1", j)
            lab = Label(lab.r, lab.stage, (0, 1, 2), tgt[:3], "r1_zero")
        else:
            for w, v in zip(lab.words, lab.values):
                tgt[w] = v
            if lab.kind == "held_zero" and not any(lab.values):      # no constant deferred here: a true zero
                lab = Label(lab.r, lab.stage, lab.words, lab.values, "zero")
            key = tuple(lab[:4])
        if key in seen:
            continue
        seen.add(key)
        out.append((input_for(lab.r, lab.stage, tgt), lab))
    return tuple(out)


def r1_rows(lab: Label) -> list:
    """The gadget rows j whose r1 wire (M[j][0] z0 + M[j][1] z1 + M[j][2] z2 at "mds_in") an "r1_zero" entry makes zero."""
    mds = S.mds_matrix()
    z = lab.values
    return [j for j in range(WIDTH) if (mds[j][0] * z[0] + mds[j][1] * z[1] + mds[j][2] * z[2]) % P == 0]
