"""CPU tier: the form table of tests/gpu_common.py (which kernel a sponge / absorb / Merkle level / verify / update call runs
for a given size) agrees with the library's exported size rule at every threshold, +-1, and each size list the GPU tests
draw from reaches the form it names.  No compute call is made."""
import pytest

from gpu_common import (COOP_MAX, COUNT_GRID_RECORDS, FORM_SIZES, LANES_HELPED_MAX, LANES_MAX, LEVEL_SIZES, ROWS_MAX,
                        absorb_form, form_family, level_form, sponge_form, update_form, verify_form)

KERNEL_LANES, KERNEL_ROWS, KERNEL_COOP, KERNEL_FAST = 4, 5, 3, 2
FAMILY = {"lanes": KERNEL_LANES, "rows": KERNEL_ROWS, "coop": KERNEL_COOP, "fast": KERNEL_FAST}
EDGES = sorted({max(1, t + d) for t in (1, LANES_HELPED_MAX, LANES_MAX, ROWS_MAX, COOP_MAX, COUNT_GRID_RECORDS)
                for d in (-1, 0, 1)})


def chain_forms(n, arity=4):
    return [sponge_form(n)[-1], absorb_form(n), verify_form(n, arity), update_form(n, arity), level_form(n * arity, arity)]


@pytest.mark.parametrize("n", EDGES)
def test_form_table_matches_the_library(hades_lib, n):
    sel = hades_lib.hades252_chain_form_for(n)
    assert sel == hades_lib.hades252_kernel_for(n)
    fam = hades_lib.hades252_kernel_name(sel, n).decode()
    assert fam == "k_perm_" + {v: k for k, v in FAMILY.items()}[sel]
    for arity in (2, 3, 4):
        for name in chain_forms(n, arity):
            assert FAMILY[form_family(name)] == sel, (n, arity, name)
    helped = n <= LANES_HELPED_MAX
    assert sponge_form(n)[-1] == "k_sponge_lanes<%s>" % ("true" if helped else "false") or n > LANES_MAX


@pytest.mark.parametrize("n", EDGES)
def test_sort_only_above_coop_max(n):
    plain = sponge_form(n)
    srt = sponge_form(n, sorted=True)
    assert srt[-1] == plain[-1]
    if n > COOP_MAX:
        assert srt == ("k_sponge_count", "k_sponge_scan", "k_sponge_scatter", "k_sponge")
    else:
        assert srt == plain


def test_ragged_levels_above_rows_run_per_lane():
    for arity in (2, 3, 4):
        for parents in (ROWS_MAX + 1, 9001, COOP_MAX):
            assert level_form(parents * arity, arity) == "k_merkle_coop<%d>" % arity
            assert level_form(parents * arity - 1, arity) == "k_merkle_level_fast<%d>" % arity
        assert level_form(ROWS_MAX * arity - 1, arity) == "k_merkle_rows<%d>" % arity
        assert level_form((COOP_MAX + 1) * arity, arity) == "k_merkle_level_fast<%d>" % arity
    assert level_form(9001, 1) == "k_merkle_coop<1>"           # arity 1 is never ragged


def test_size_lists_reach_their_forms():
    want = {"lanes_helped": "k_sponge_lanes<true>", "lanes": "k_sponge_lanes<false>", "rows": "k_sponge_rows",
            "coop": "k_sponge_coop", "fast": "k_sponge"}
    assert set(FORM_SIZES) == set(want)
    for form, sizes in FORM_SIZES.items():
        assert len(sizes) == 3 and sizes[0] < sizes[1] < sizes[2]
        for n in sizes:
            assert sponge_form(n) == (want[form],), (form, n)
            assert form_family(absorb_form(n)) == form_family(want[form])
        # first size and last size sit on the form's boundaries; the middle one is ragged (no multiple of 64)
        assert sizes[1] % 64 != 0
        assert sizes[0] == 1 or sponge_form(sizes[0] - 1) != (want[form],)
        if form != "fast":
            assert sponge_form(sizes[2] + 1) != (want[form],)
    for arity in (2, 3, 4):
        for form, sizes in LEVEL_SIZES.items():
            for parents in sizes:
                n_children = parents * arity - (1 if form == "fast_ragged" else 0)
                got = level_form(n_children, arity)
                assert form_family(got) == ("fast" if form == "fast_ragged" else form_family(want[form])), (form, parents)
                assert got.endswith("true>") == (form == "lanes_helped")
            for nq in FORM_SIZES.get(form, ()):
                assert form_family(verify_form(nq, arity)) == form_family(update_form(nq, arity)) == form_family(want[form])
