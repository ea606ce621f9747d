"""The per-entity ALS checks of tests/als_step_ref.py, themselves tested on the CPU: the longdouble reference agrees with
oracle/als_oracle.py half by half, the float64 kernel-order restatement stays within K / 8 of it on every case of
tests/als_cases.py (that measurement is where K comes from), and the restatement with one planted fault is rejected."""
import numpy as np
import pytest

from oracle.als_oracle import AlsOracle
from tests import als_cases as C
from tests import als_step_ref as S

REDUCED = dict(nu=700, nw=6, n=6000)                       # grid_stride's shape at a size the CPU restatement walks


def _oracle_halves(nu, nw, d, lam, u, w, y, bias, tables):
    """one AlsOracle sweep as its two halves: (state after the user loop, state after the work loop)"""
    o = AlsOracle(nu, nw, d, 1, lam)
    o.load(np.stack([u, w], 1), y)
    o.U, o.V, o.W_user, o.W_work = (np.array(t) for t in tables)
    o.bias = bias
    for e in o.users:
        o._fit(o.U, o.V, o.W_user, o.W_work, o.by_user, e)
    mid = dict(U=o.U.copy(), W_user=o.W_user.copy())
    for e in o.works:
        o._fit(o.V, o.U, o.W_work, o.W_user, o.by_work, e)
    return o, dict(mid, V=o.V, W_work=o.W_work)


def _golden_case(g, name):
    nu, nw, d, _ = (int(x) for x in g[name + "/shape"])
    X, y = np.asarray(g[name + "/X"], np.int64), np.asarray(g[name + "/y"], np.float64)
    rs = np.random.RandomState(7)
    return dict(id="golden-" + name, d=d, lam=float(g[name + "/lam"]), bias=float(y.mean()), ch=None, nu=nu, nw=nw,
                u=np.ascontiguousarray(X[:, 0]), w=np.ascontiguousarray(X[:, 1]), y=y,
                U=rs.rand(nu, d), V=rs.rand(nw, d), Wu=rs.rand(nu), Ww=rs.rand(nw))


@pytest.mark.parametrize("name", ["small", "d8", "tile_edges-d20", "tile_edges-d20-swapped"])
def test_the_reference_agrees_with_the_oracle_half_by_half(golden, name):
    """AlsOracle solves by LU in float64: it is held to the same bound the device is, at K"""
    if name.startswith("tile"):
        case = C.tile_edges(20)
        case = C.swapped(case) if name.endswith("swapped") else case
    else:
        case = _golden_case(golden("als_trajectory.npz"), name)
    o, after = _oracle_halves(case["nu"], case["nw"], case["d"], case["lam"], case["u"], case["w"], case["y"], case["bias"],
                              (case["U"], case["V"], case["Wu"], case["Ww"]))
    (lu, users), (lw, works) = S.sides(case)
    assert np.array_equal(users, o.users) and np.array_equal(works, o.works)
    for mine, theirs in ((lu, o.by_user), (lw, o.by_work)):
        assert all(np.array_equal(a, b) for a, b in zip(mine, theirs))
    report = {}
    bad = S.check_sweep(case, after, S.K, report)
    print("RATIO %s oracle against the reference: %s" % (case["id"], report))
    assert not bad, "\n".join(bad)


def _all_cases():
    reduced = C.grid_stride(**REDUCED)
    return C.CASES + [reduced, C.swapped(reduced)]


def test_the_restatement_stays_within_an_eighth_of_K_on_every_case():
    """The measurement behind K: the largest rho_x and rho_w of the float64 kernel-order restatement over every case, both
    orientations, both halves.  K = 8 * max rounded up is recorded in tests/als_step_ref.py; this test keeps later cases
    from outgrowing it."""
    worst = dict(x=(0.0, None), w=(0.0, None))
    bad = []
    for case in _all_cases():
        report = {}
        bad += S.check_sweep(case, S.sweep_f64(case), S.K / 8.0, report)
        for what, (rx, rw) in report.items():
            print("RATIO %-40s %s rho_x %.3f rho_w %.3f" % (case["id"], what, rx, rw))
            worst["x"] = max(worst["x"], (rx, case["id"] + ", " + what), key=lambda t: t[0])
            worst["w"] = max(worst["w"], (rw, case["id"] + ", " + what), key=lambda t: t[0])
    print("MEASURED max rho_x %.3f (%s), max rho_w %.3f (%s), K = %g" % (worst["x"] + worst["w"] + (S.K,)))
    assert not bad, "\n".join(bad)
    assert abs(worst["x"][0] - S.MEASURED_RHO_X) < 1e-3 and abs(worst["w"][0] - S.MEASURED_RHO_W) < 1e-3, "not the recorded maxima"
    assert S.K == int(np.ceil(8 * max(S.MEASURED_RHO_X, S.MEASURED_RHO_W)))


def _case(cid):
    return [c for c in C.CASES if c["id"] == cid][0]


# fault -> (case, what a violated statement must contain)
FAULTS = {
    "drop_partial_tile": ("tile_edges-d9", "user half x"),
    "skip_slot3": ("tile_edges-d28", "user half x"),
    "drop_last_chunk": ("chunk_edges-ch32-d9", "user half x"),
    "n_minus_1": ("tile_edges-d9-swapped", "user half x"),
    "fit_all_zero": ("sweep_sets", "outside the sweep set changed"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_are_rejected(fault):
    """Each of these errors, planted in the restatement's sweep, violates a statement of the half it sits in:

      drop_partial_tile  a list's last tile of fewer than 32 ratings left out of A and b
      skip_slot3         the A entries 768 .. d*d - 1 (the fourth accumulator slot, live from d = 28) never accumulated
      drop_last_chunk    a chunked list's last chunk left out of the sum of partial sums
      n_minus_1          lambda (N - 1) on the diagonal
      fit_all_zero       entities whose ratings are all 0.0 fitted like the others"""
    cid, text = FAULTS[fault]
    case = _case(cid)
    assert S.check_sweep(case, S.sweep_f64(case), S.K) == []
    bad = S.check_sweep(case, S.sweep_f64(case, fault), S.K)
    print("fault %s: %d statements violated, first: %s" % (fault, len(bad), bad[:1]))
    assert any(text in b for b in bad), "fault %s passes, or no statement holds %r: %s" % (fault, text, bad)


def test_cases_hold_what_they_are_built_for():
    from tests import widths as W
    by_id = {c["id"]: c for c in C.CASES}
    assert len(by_id) == len(C.CASES)
    for d in W.ALS_STEP:
        for cid in ("tile_edges-d%d" % d, "tile_edges-d%d-swapped" % d):
            c = by_id[cid]
            (lu, users), (lw, works) = S.sides(c)
            lists = lu if not cid.endswith("swapped") else lw
            assert set(C.TILE_LENGTHS) <= set(np.diff(lists[0]).tolist())
            dup = lists[1][lists[0][13]:lists[0][14]]
            assert dup.size == 5 and np.unique(dup).size == 4          # one partner rated twice, both kept
            assert c["bias"] != c["y"].mean()
    for ch, d in C.CHUNK_CASES:
        c = by_id["chunk_edges-ch%d-d%d" % (ch, d)]
        (lu, _), (lw, _) = S.sides(c)
        nu, nw = S.n_chunks(lu, S.chunk_size(c["ch"])), S.n_chunks(lw, S.chunk_size(c["ch"]))
        assert {ch, ch + 1, 2 * ch, 2 * ch + 1, 3 * ch - 1, 1, 5, 31} <= set(np.diff(lu[0]).tolist())
        assert nu.sum() == 2 + 2 + 3 + 3 and nw.sum() == 2 and nu[0] == 0                # N = ch is not chunked
        plain = by_id["chunk_edges-ch%d-d%d-unchunked" % (ch, d)]
        assert plain["ch"] is None and S.n_chunks(lu, S.chunk_size(None)).sum() == 0
        assert all(np.array_equal(plain[k], c[k]) for k in ("u", "w", "y", "U", "V", "Wu", "Ww"))
    c = by_id["sweep_sets"]
    (lu, users), (lw, works) = S.sides(c)
    assert users.tolist() == [1, 3, 4, 5, 6, 7] and 8 not in works and 9 not in works
    assert np.diff(lu[0])[[0, 1, 2]].tolist() == [3, 2, 0] and np.diff(lw[0])[[8, 9]].tolist() == [1, 0]
    assert any(0 in lw[1][lw[0][e]:lw[0][e + 1]] for e in works)       # a fitted work reads the unfitted user's row
    for lam in C.LAMBDAS:
        c = by_id["conditioning-lam%g" % lam]
        assert c["d"] == 32 and np.diff(S.sides(c)[0][0][0]).tolist() == [1, 5, 31, 40]
    r = C.grid_stride(**REDUCED)
    assert r["ch"] == 32 and r["d"] == 2 and S.n_chunks(S.sides(r)[1][0], 32).min() > 2
