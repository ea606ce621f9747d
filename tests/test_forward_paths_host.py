"""The forward-path cases held to their claims on the CPU (tests/forward_cases.py; the GPU side is
tests/test_gpu_forward_paths.py): the 256 MB rule as tfr_forward_plan reports it, the big-table embedding of the exact
case, and the random case's distance from the rounding edge of the nll head."""
import numpy as np
import pytest

from tests import bf16_cases as BC
from tests import forward_cases as F
from tests import widths as W
from tests.util import make_oracle

ROWS = [(F.F32, D) for D in W.FORWARD_PNT] + [(F.BF16, D) for D in W.BF16_PNT]


@pytest.fixture(autouse=True)
def no_override(monkeypatch):
    monkeypatch.delenv("TFR_BF16_PNT", raising=False)


# ---------------------------------------------------------------- the plan entry
def test_plan_names_the_kernel_and_the_grid():
    assert F.plan_text(128, 1000, F.INFER, F.F32, 1000) == (0, "k_forward<32, 4, 0, 4, false>;grid=32")
    assert F.plan_text(15, 1000, F.EVAL, F.F32, 10 ** 7) == (0, "k_forward<16, 1, 2, 4, false>;grid=2048")
    assert F.plan_text(15, 1000, F.TRAIN, F.F32, 1) == (0, "k_forward<16, 1, 1, 4, false>;grid=1")
    assert F.plan_text(100, 1000, F.INFER, F.BF16, 10 ** 7) == (0, "k_forward_bf16<16, 0, 4, false>;grid=8192")
    assert F.plan_text(9, 1000, F.EVAL, F.BF16, 0) == (0, "k_forward_bf16<2, 2, 2, false>;grid=1")
    assert F.plan_text(1, 1000, F.INFER, F.BF16, 257) == (0, "k_forward_bf16<1, 0, 1, false>;grid=2")


@pytest.mark.parametrize("rows,D", ROWS)
def test_grid_is_the_batch_in_blocks_up_to_the_cap(rows, D):
    pb = F.per_block(D) if rows == F.F32 else BC.per_block(D)
    for mode, cap in ((F.INFER, F.INFER_CAP), (F.EVAL, F.EVAL_CAP)):
        for B, want in ((1, 1), (pb, 1), (pb + 1, 2), (cap * pb, cap), (cap * pb + 1, cap)):
            assert F.plan(D, 1000, mode, rows, B)[2] == want, (rows, D, mode, B)


def test_plan_refuses_what_no_forward_runs():
    from tfrecomm_amd import _lib as L
    for args in ((65, 10, F.INFER, F.F32, 1), (0, 10, F.INFER, F.F32, 1), (260, 10, F.EVAL, F.BF16, 1),
                 (64, 10, F.TRAIN, F.BF16, 1), (64, 10, 3, F.F32, 1), (64, 10, F.INFER, 2, 1), (64, 0, F.INFER, F.F32, 1),
                 (64, 10, F.INFER, F.F32, -1)):
        assert F.plan_text(*args)[0] == L.ERR_ARG, args
    rc, text = F.plan_text(64, 10, F.INFER, F.F32, 1)
    assert rc == 0
    assert F.plan_text(64, 10, F.INFER, F.F32, 1, buflen=len(text))[0] == L.ERR_ARG          # no room for the terminator
    assert F.plan_text(64, 10, F.INFER, F.F32, 1, buflen=len(text) + 1) == (0, text)
    assert L.load().tfr_forward_plan(64, 10, F.INFER, F.F32, 1, None, 128) == L.ERR_ARG


@pytest.mark.parametrize("rows,D", ROWS)
def test_pnt_rows_is_the_first_table_above_256_mb(rows, D):
    rb = F.row_bytes(D, rows)
    U = F.pnt_rows(D, rb)
    assert U * rb > 256 << 20 >= (U - 1) * rb
    for mode in (F.INFER, F.EVAL):
        assert F.plan_pnt(D, U, mode, rows) is True and F.plan_pnt(D, U - 1, mode, rows) is False


def test_the_snapshot_override_is_read_at_every_call(monkeypatch):
    U = F.pnt_rows(100, F.row_bytes(100, F.BF16))
    monkeypatch.setenv("TFR_BF16_PNT", "1")
    assert F.plan_pnt(100, 40, F.INFER, F.BF16) is True and F.plan_pnt(100, 40, F.EVAL, F.BF16) is True
    assert F.plan_pnt(100, F.pnt_rows(100, 400) - 1, F.INFER, F.F32) is False    # the float32 rows do not read it
    monkeypatch.setenv("TFR_BF16_PNT", "0")
    assert F.plan_pnt(100, U, F.INFER, F.BF16) is False
    monkeypatch.setenv("TFR_BF16_PNT", "yes")                                    # neither 0 nor 1: the rule
    assert F.plan_pnt(100, U, F.INFER, F.BF16) is True and F.plan_pnt(100, U - 1, F.INFER, F.BF16) is False


# ---------------------------------------------------------------- rows of a big table
@pytest.mark.parametrize("U,rb", [(F.pnt_rows(3, 12), 12), (F.pnt_rows(256, 1024), 1024), ((1 << 21) + 2, 1024),
                                  ((1 << 22) + 2, 512), (40, 12), (3 * (1 << 28) // 244, 244)])
def test_spread_rows_reach_both_ends_and_both_byte_offsets(U, rb):
    pos = F.spread_rows(U, rb, 40)
    assert pos.shape == (40,) and (np.diff(pos) > 0).all() and pos[0] == 0 and pos[-1] == U - 1
    for off in (1 << 28, 1 << 31):
        if U * rb > off + rb:
            first, last = pos * rb, pos * rb + rb - 1       # the bytes a row covers
            assert ((last < off) & (last >= off - 2 * rb)).any() and ((first >= off) & (first < off + 2 * rb)).any(), (U, rb, off)
            assert ((first <= off) & (off <= last)).any()   # and the row that holds the offset itself
    assert np.array_equal(pos, F.spread_rows(U, rb, 40))


@pytest.mark.parametrize("rows,D", ROWS)
def test_embedded_exact_case_is_exact_in_any_order(rows, D):
    item_abs = bool((W.FORWARD_PNT if rows == F.F32 else W.BF16_PNT).index(D) & 1)
    rb = F.row_bytes(D, rows)
    U = F.pnt_rows(D, rb)
    t, u, i, r, want, sse, neq = BC.exact_reference(D, item_abs)
    big, ub, i2, r2, want2, sse2, neq2, pos = F.exact_big_case(D, item_abs, U, rb)
    assert big["P"].shape == (U, D) and big["bu"].shape == (U,) and ub.dtype == np.int32
    assert {0, U - 1} <= set(pos.tolist()) and np.array_equal(pos, F.spread_rows(U, rb, 40))
    assert np.array_equal(big["P"][pos], t["P"]) and np.array_equal(big["bu"][pos], t["bu"])
    assert np.count_nonzero(big["P"]) == np.count_nonzero(t["P"]) and np.count_nonzero(big["bu"]) == np.count_nonzero(t["bu"])
    assert np.array_equal(ub, pos[u]) and {0, U - 1} <= set(ub.tolist())       # both ends of the table are read
    assert F.embedded_faults(big, ub, i, r, item_abs) == []
    # the same ratings: the float64 values of the embedded case are those of the case it came from
    assert np.array_equal(BC.exact_logits(big, ub, i, item_abs).astype(np.float32), want)
    assert BC.exact_eval(big, ub, i, r, item_abs) == (sse, neq) == (sse2, neq2) and 0 < neq < len(u)


def test_embedded_guard_fails_on_a_planted_third():
    D, item_abs = 13, False
    U = F.pnt_rows(D, 4 * D)
    big, ub, i, r, _, _, _, pos = F.exact_big_case(D, item_abs, U, 4 * D)
    k = int(np.flatnonzero(big["Q"][i, 0] != 0)[0])
    big["P"][ub[k], 0] = np.float32(1.0 / 3.0)
    assert "rows are bf16-exact integers" in F.embedded_faults(big, ub, i, r, item_abs)
    big2, ub2, _, _, _, _, _, _ = F.exact_big_case(D, item_abs, U, 4 * D)
    big2["P"][1, 0] = np.float32(1.0 / 3.0)                # a row no rating reads still belongs to the table
    assert 1 not in pos and "rows are bf16-exact integers" in F.embedded_faults(big2, ub2, i, r, item_abs)


def test_canary_rows_follow_the_filled_rows_and_no_rating_reads_them():
    D = 61
    U = F.pnt_rows(D, 4 * D)
    big, ub, i, r, want, _, _, pos = F.exact_big_case(D, True, U, 4 * D)
    canaries = F.plant_canaries(big, pos)
    assert len(canaries) >= 30 and np.isin(canaries - 1, pos).all() and not np.isin(canaries, pos).any() and canaries.max() < U
    assert np.isnan(big["P"][canaries]).all() and np.count_nonzero(np.isnan(big["P"]).any(axis=1)) == len(canaries)
    assert np.array_equal(BC.exact_logits(big, ub, i, True).astype(np.float32), want)          # none of them is read
    # what an unguarded lane would add: the first element of the next row times the item side's zero
    assert np.isnan(np.float32(big["P"][pos[0] + 1, 0]) * np.float32(0))


# ---------------------------------------------------------------- the random case
@pytest.mark.parametrize("D", sorted(set(W.FORWARD_PNT) | set(W.BF16_PNT) | set(W.SVD_SMALL)))
@pytest.mark.parametrize("item_abs", [False, True])
def test_random_case_has_no_logit_at_the_rounding_edge(D, item_abs):
    t, u, i, r = F.random_case(D, "nll", item_abs)
    n, I = BC.EXACT_TABLES[0], F.RANDOM_I
    assert t["P"].shape == (n, D) and len(u) >= 3 * F.per_block(D) + 5 and set(np.unique(r)) == {0.0, 1.0}
    for tables in (t, BC.snapshot_tables(t)):
        x = make_oracle(n, I, D, tables, loss="nll", item_abs=item_abs).forward(u, i)
        assert np.abs(x).min() >= 1e-4, (D, item_abs, np.abs(x).min())
    t2, u2, i2, r2 = F.random_case(D, "mse", item_abs)
    assert np.array_equal(t2["P"], t["P"]) and np.array_equal(u2, u) and set(np.unique(r2)) <= {1.0, 2.0, 3.0, 4.0, 5.0}


def test_grid_stride_widths_are_one_scalar_and_one_vector_geometry_below_full_width():
    vecs = {F.geometry(D)[1] for D in F.GRID_STRIDE}
    assert vecs == {1, 4} and all(D in W.FORWARD_PNT and D != F.geometry(D)[0] * F.geometry(D)[1] for D in F.GRID_STRIDE)
