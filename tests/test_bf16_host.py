"""The bf16 snapshot's number format, row layout and lane geometry, checked on the CPU (tfrecomm_amd/bf16.py restates
csrc/bf16_rows.h; the GPU side is tests/test_gpu_bf16.py)."""
import numpy as np
import pytest

from tfrecomm_amd import bf16
from tests import bf16_cases as C
from tests.util import make_oracle


def test_to_bits_is_torchs_conversion_bit_for_bit():
    x = np.concatenate([C.random_values(), C.EDGE_BITS.view(np.float32)])
    assert x.size == 202000 + C.EDGE_BITS.size
    assert (np.abs(x[:202000]) > 3.0e38).any() and (np.abs(x[:202000]) < 1e-38).any()
    got, want = bf16.to_bits(x), C.torch_bits(x)
    assert got.dtype == np.uint16 and np.array_equal(got, want)


def test_edge_list_rounds_as_stated():
    h = dict(zip(C.EDGE_BITS.tolist(), bf16.to_bits(C.EDGE_BITS.view(np.float32)).tolist()))
    assert h[0x3F808000] == 0x3F80 and h[0x3F818000] == 0x3F82                       # ties to even: down, up
    assert h[0x3F807FFF] == 0x3F80 and h[0x3F808001] == 0x3F81 and h[0x3F817FFF] == 0x3F81 and h[0x3F818001] == 0x3F82
    assert h[0x7F7F8000] == 0x7F80 and h[0x7F7F7FFF] == 0x7F7F and h[0xFF7F8000] == 0xFF80
    assert h[0x00008000] == 0x0000 and h[0x80008000] == 0x8000                       # half of the smallest: tie to even
    assert h[0x00008001] == 0x0001 and h[0x80008001] == 0x8001 and h[0x00007FFF] == 0x0000
    assert h[0x00000000] == 0x0000 and h[0x80000000] == 0x8000 and h[0x7F800000] == 0x7F80 and h[0xFF800000] == 0xFF80


def test_nan_stays_nan_with_its_sign():
    h = bf16.to_bits(C.NAN_BITS.view(np.float32))
    back = bf16.from_bits(h)
    assert np.isnan(back).all()
    assert np.array_equal(h >> 15, (C.NAN_BITS >> 31).astype(np.uint16))
    assert ((h & 0x0040) != 0).all()                                                 # quiet


def test_round_trip_is_the_identity_on_bf16_values():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = bf16.from_bits(h)
    keep = ~np.isnan(x)
    assert np.array_equal(bf16.to_bits(x[keep]), h[keep])
    assert np.array_equal(bf16.round_trip(x[keep]).view(np.uint32), x[keep].view(np.uint32))
    assert np.isnan(bf16.round_trip(x[~keep])).all()


@pytest.mark.parametrize("D", C.WIDTHS)
def test_pack_rows_pads_with_plus_zero(D):
    t = np.random.RandomState(D).normal(0, 0.3, (5, D)).astype(np.float32)
    p = bf16.pack_rows(t)
    DP = C.row_stride(D)
    assert p.shape == (5, DP) and p.dtype == np.uint16 and DP % 8 == 0 and 0 <= DP - D < 8
    assert np.array_equal(p[:, :D], bf16.to_bits(t)) and not p[:, D:].any()
    assert bf16.row_stride(D) == DP and bf16.lanes(D) == C.lanes(D)


# ---------------------------------------------------------------- geometry
def supported(D):
    """a row width the model accepts (csrc/svd_kernels.h geometry)"""
    return 1 <= D <= 64 or (D % 4 == 0 and D <= 256)


def width_class(D):
    """(lanes per rating, every lane of the group holds a fragment, pad elements): k_forward_bf16<G, ...> is picked by
    G; lanes past DP / 8 take the redirected load and the zeroed sum; the pad decides what k_rows_to_bf16 zero-fills and
    whether its second 16-byte load is skipped (D % 8 == 4)"""
    return C.lanes(D), C.lanes(D) * 8 == C.row_stride(D), C.row_stride(D) - D


def test_widths_reach_every_lane_group_size_and_kind_of_pad():
    assert all(supported(D) for D in C.WIDTHS)
    assert {C.lanes(D) for D in range(1, 257) if supported(D)} == {1, 2, 4, 8, 16, 32}
    classes = [width_class(D) for D in C.WIDTHS]
    assert len(set(classes)) == len(classes), "two widths reach the same class: one of them guards nothing"
    want = set()
    for g in (1, 2, 4, 8, 16, 32):
        want.add((g, True, 0))                                     # the group's upper end: full width, no pad
    for g in (1, 2, 4, 8):
        lo = 1 if g == 1 else 4 * g + 1                            # the group's lower end: the longest pad, and past
        want.add(width_class(lo))                                  # G = 2 lanes without a fragment
        want.add((g, True, 1))                                     # one below the upper end: the shortest pad
    for g in (16, 32):                                             # D % 4 == 0 only: the pad is 0 or 4
        want.add((g, False, 4))
    want |= {(32, True, 4), (32, False, 0)}
    assert want == set(classes), (sorted(want - set(classes)), sorted(set(classes) - want))
    assert {C.unroll(C.lanes(D)) for D in C.WIDTHS} == {1, 2, 4}
    assert C.per_block(128) == 64                                  # what the grid-stride case sizes its batches by


# ---------------------------------------------------------------- quantisation bound
@pytest.mark.parametrize("D", [1, 8, 64, 256])
def test_quantisation_bound_holds_and_half_of_it_does_not(D):
    rs = np.random.RandomState(100 + D)
    n = 20000
    p, q = rs.normal(0, 0.3, (n, D)).astype(np.float32), rs.normal(0, 0.3, (n, D)).astype(np.float32)
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    ph, qh = bf16.round_trip(p).astype(np.float64), bf16.round_trip(q).astype(np.float64)
    diff = np.abs((ph * qh).sum(1) - (p64 * q64).sum(1))
    scale = (np.abs(p64) * np.abs(q64)).sum(1)
    worst = float((diff / scale).max() / C.QBOUND)
    print("D = %d: worst |dot_bf16 - dot_f32| = %.3f of the bound" % (D, worst))
    assert (diff <= C.QBOUND * scale).all()
    if D == 1:
        # the planted fault: a bound set at half this value has to fail, or the bound above checks nothing
        assert not (diff <= 0.5 * C.QBOUND * scale).all()
        assert worst > 0.8


# ---------------------------------------------------------------- the eval case of the GPU tests
def test_eval_case_has_no_logit_at_the_rounding_edge():
    U, I, D, N = C.EVAL_SHAPE
    t, u, i, _ = C.eval_case("nll")
    x = make_oracle(U, I, D, C.snapshot_tables(t), loss="nll").forward(u, i)
    assert np.abs(x).min() >= 1e-4, np.abs(x).min()


# ---------------------------------------------------------------- the exact case of the GPU tests
@pytest.mark.parametrize("item_abs", [False, True])
@pytest.mark.parametrize("D", C.WIDTHS)
def test_exact_case_is_exact_in_any_order(D, item_abs):
    t, u, i, r = C.exact_case(D, item_abs)
    assert len(u) == 3 * C.per_block(D) + 5
    assert C.exactness_faults(t, u, i, r, item_abs) == []
    x = C.exact_logits(t, u, i, item_abs)
    sse, neq = C.exact_eval(t, u, i, r, item_abs)
    assert 0 < neq < len(u) and sse > 0                            # both counts of the evaluation are at work
    assert len(np.unique(x)) > 20 and (x != np.rint(x)).any()      # the half-valued biases reach the logits
    if item_abs:
        assert not np.array_equal(x, C.exact_logits(t, u, i, False))


def test_exactness_guard_fails_on_a_planted_third():
    D, item_abs = 100, False
    t, u, i, r = C.exact_case(D, item_abs)
    k = int(np.flatnonzero(t["Q"][i, 0] != 0)[0])
    t["P"] = t["P"].copy()
    t["P"][u[k], 0] = np.float32(1.0 / 3.0)                        # neither an integer nor bf16-exact
    faults = C.exactness_faults(t, u, i, r, item_abs)
    assert "rows are bf16-exact integers" in faults
    assert "float32 logits in two orders equal float64" in faults  # the orders do differ: the guard sees it by evaluation
