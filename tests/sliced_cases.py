"""The cases of the scoring block's exact tests (tests/test_sliced_block_ref_host.py, tests/test_gpu_sliced_block.py).

A case is a table set, query rows, k and exclusions.  Every score is exact in f32, so the device must return the contract's
ids and score bits (tests/topk_ref.py), and every query's score row has a chosen shape:

- The rows repeat NU = 32 distinct users.  User u's P row is c(u) on feature f(u) = u % D and zero elsewhere, with
  c(u) = (1, -1, 1/2, -2)[u // D % 4]; column f of Q holds pattern f over the item ids (``PATTERNS``): integers or eighths
  below 2^21, so ((c q + mu) + bu) + bi is exact.  A ramp under c < 0 is the descending ramp, and so on.
- mu, bu and bi are small dyadics.  bi is one constant unless the case carries the special values (``bi="specials"``):
  a whole round of NaN, a whole slice of NaN, +inf, -inf and -0 (which, added to a score, changes nothing: no score of
  these formulas can be -0, the accumulators start from +0; the model's own test orders +0 against -0).
- With ``excl`` four users have exclusions: user 0 (ascending ramp) loses the top of its ramp (a long row, hit in the late
  rounds), user D + 0 (descending ramp) the top of its own (hit in round one), user 1 everything, and user 2 all but
  k // 2 + 3 items spread over the slices (padding, and a merge that runs out of keys).  The others have empty rows.
- Every tile of 16 or 32 rows mixes the users, one user appears twice in it, and the row count leaves the last tile partial.

``slices`` / ``rounds`` are what a case claims of the launch plan; both test files check the claim against the restated
plan and the GPU file against tfr_topk_plan, so a change of the constants fails there instead of emptying a case."""
import functools

import numpy as np

from tests import sliced_block_ref as M
from tests.topk_ref import svd_scores, topk_ref

NU = 32
MULTS = (1.0, -1.0, 0.5, -2.0)
MU = np.float32(0.25)
BI_CONST = np.float32(0.5)

PATTERNS = ("ascending", "constant", "plateaus", "spikes", "random", "sawtooth", "round_tops", "late_kth", "scrambled")


def pattern(name, I, rs, k):
    i = np.arange(I, dtype=np.int64)
    if name == "ascending":                                # every candidate beats the threshold
        return 4.0 * i
    if name == "constant":                                 # ties by id alone, against a threshold of equal score
        return np.full(I, 3.0)
    if name == "plateaus":                                 # runs of 80 equal scores: across round and slice boundaries
        return (i // 80).astype(np.float64)
    if name == "spikes":                                   # one spike per 128 items: per slice where a slice is one round
        return np.where(i % 128 == 77, 5000.0 + (i // 128) % 7, (i % 13) * 0.25)
    if name == "random":
        return rs.randint(-1024, 1025, I) * 0.125
    if name == "sawtooth":                                 # every value 128 apart in id: ties across rounds and lists
        return (i % 251).astype(np.float64)
    if name == "round_tops":                               # the last lanes of every round win: a few appends per round
        return ((i % 128) * 1024 + i // 128).astype(np.float64)
    if name == "scrambled":                                # no ties, no order
        return ((i * 2654435761) % (1 << 20)).astype(np.float64)
    if name == "late_kth":
        # A ramp over the first T items, which ends with the round after which slice 0's queues compact (CAP 256: round 2;
        # CAP 512: round 4) holding the ramp's k best; everything later is low, but for one item X of a later round that
        # scores between the k-th and the (k - 1)-th of them: only a threshold that is exactly the k-th key lets it in
        # and only a cut at exactly k keeps it.
        T, X = (256, 263) if M.topk_cap(k) == 256 else (512, 647)
        if I <= X:
            return 4.0 * i
        v = np.where(i < T, 4.0 * i, -1.0 - i % 5)
        v[X] = 4.0 * (T - k) + 2
        return v
    raise KeyError(name)


class Case:
    def __init__(self, name, group, I, D, k, n_rows, slices, rounds, bi="const", excl=True, row_users=None, seed=0):
        self.name, self.group, self.I, self.D, self.k, self.n_rows = name, group, I, D, k, n_rows
        self.slices, self.rounds = slices, rounds          # claimed: slices planned, rounds of each (a list, or one number)
        self.bi_mode, self.with_excl, self.row_users, self.seed = bi, excl, row_users, seed

    def __repr__(self):
        return self.name

    # -- the plan ------------------------------------------------------------------------------------------------------
    def plan(self, n_rows=None, cand=None):
        return M.topk_plan(self.k, self.n_rows if n_rows is None else n_rows, self.I if cand is None else cand)

    def claimed_rounds(self):
        r = self.rounds
        return list(r) if isinstance(r, (list, tuple)) else [r] * self.slices

    # -- tables ----------------------------------------------------------------------------------------------------------
    def user_feature(self, u):
        return u % self.D

    def user_mult(self, u):
        return MULTS[u // self.D % 4]

    @functools.lru_cache(maxsize=None)
    def tables(self):
        rs = np.random.RandomState(1000 + self.seed)
        I, D = self.I, self.D
        Q = np.stack([pattern(PATTERNS[f], I, rs, self.k) for f in range(D)], 1).astype(np.float32)
        P = np.zeros((NU, D), np.float32)
        for u in range(NU):
            P[u, self.user_feature(u)] = self.user_mult(u)
        bu = (0.25 * (np.arange(NU) % 5)).astype(np.float32)
        bi = np.full(I, BI_CONST, np.float32)
        if self.bi_mode == "specials":
            p = self.plan()
            per = M.slice_bounds(p, 0, I, 0)[0]
            if I > 256:
                bi[128:256] = np.nan                       # a whole round of slice 0
            if p["slices"] > 1 and 2 * per <= I:
                bi[per:2 * per] = np.nan                   # the whole of slice 1
            mid = min(I - 1, (p["slices"] // 2) * per + 3)
            bi[[5, mid, I - 1]] = np.inf
            bi[[7, I - 2]] = -np.inf
            bi[[9, I - 3]] = -0.0
        t = dict(mu=MU, bu=bu, bi=bi, P=P, Q=Q)
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return t

    # -- rows and exclusions -----------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def rows(self):
        if self.row_users is not None:
            r = np.asarray(self.row_users, np.int32)
            assert r.size == self.n_rows
        else:
            r = np.arange(self.n_rows)
            r = ((r + 3 * (r // NU)) % NU).astype(np.int32)
            twice = np.flatnonzero(np.arange(self.n_rows) % 16 == 5)
            r[twice] = r[twice - 2]                        # a user twice in one tile
        r.setflags(write=False)
        return r

    @functools.lru_cache(maxsize=None)
    def excl_of_user(self, u):
        """sorted int32 ids user u may not be given"""
        I, k, D = self.I, self.k, self.D
        none = np.zeros(0, np.int32)
        if not self.with_excl:
            return none
        if u == 0:
            top = np.arange(max(0, I - 2 * k - 45), I)
            return top[top % 7 != 3].astype(np.int32)
        if u == D:
            return np.arange(min(I, k + 22), dtype=np.int32)
        if u == 1:
            return np.arange(I, dtype=np.int32)
        if u == 2:
            keep = np.unique(np.linspace(0, I - 1, k // 2 + 3).astype(np.int64))
            x = np.ones(I, bool)
            x[keep] = False
            return np.flatnonzero(x).astype(np.int32)
        return none

    def excl_rows(self, rows=None):
        rows = self.rows() if rows is None else rows
        return [self.excl_of_user(int(u)) for u in rows]

    def excl_csr(self, rows=None):
        if not self.with_excl:
            return None
        xs = self.excl_rows(rows)
        indptr = np.concatenate([[0], np.cumsum([x.size for x in xs])]).astype(np.int64)
        return indptr, np.concatenate(xs).astype(np.int32)

    # -- the contract's answer, once per distinct user -------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def scores(self):
        t = self.tables()
        with np.errstate(invalid="ignore"):
            S = svd_scores(t["P"], t["Q"], t["bu"], t["bi"], t["mu"], np.arange(NU))
        S.setflags(write=False)
        return S

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """(items [NU, k], scores [NU, k]) by distinct user"""
        wi, ws = topk_ref(self.scores(), self.k, [self.excl_of_user(u) for u in range(NU)])
        wi.setflags(write=False)
        ws.setflags(write=False)
        return wi, ws

    def expected(self, rows=None):
        rows = self.rows() if rows is None else rows
        wi, ws = self.reference()
        return wi[rows], ws[rows]

    @functools.lru_cache(maxsize=None)
    def simulated(self):
        """the host model's (items [NU, k], scores [NU, k], events [NU]) by distinct user"""
        p, S = self.plan(), self.scores()
        out = [M.simulate(S[u], self.k, p, self.excl_of_user(u) if self.with_excl else None) for u in range(NU)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), [o[2] for o in out]

    # -- the same case as a nearest-neighbour query: one table, the pattern rows with the users' rows put in ------------
    def nb_at(self):
        """the first of the NU query rows: they end the last slice that runs the most rounds, so the self mask meets a query
        in that slice's last round, after its queues have compacted"""
        p = self.plan()
        r = M.rounds_per_slice(p, 0, self.I)
        last = max(s for s in range(p["slices"]) if r[s] == max(r))
        return M.slice_bounds(p, 0, self.I, last)[2] - NU

    @functools.lru_cache(maxsize=None)
    def nb_table(self):
        """[I, D]: I - NU pattern rows with the NU one-feature rows of the users put in at nb_at(); query u is row
        nb_at() + u, a candidate like any other"""
        t, at = self.tables(), self.nb_at()
        T = np.concatenate([t["Q"][:at], t["P"], t["Q"][at:self.I - NU]]).astype(np.float32)
        assert T.shape[0] == self.I
        T.setflags(write=False)
        return T

    def nb_queries(self, rows=None):
        rows = self.rows() if rows is None else rows
        return (self.nb_at() + rows).astype(np.int32)

    @functools.lru_cache(maxsize=None)
    def nb_scores(self):
        from tests.neighbours_ref import neighbour_scores
        S = neighbour_scores(self.nb_table(), self.nb_at() + np.arange(NU), "dot")
        S.setflags(write=False)
        return S

    @functools.lru_cache(maxsize=None)
    def nb_reference(self):
        from tests.neighbours_ref import neighbours_from_scores
        q = self.nb_at() + np.arange(NU)
        wi, ws = neighbours_from_scores(self.nb_scores(), q, self.k, [self.excl_of_user(u) for u in range(NU)])
        return wi, ws

    @functools.lru_cache(maxsize=None)
    def nb_simulated(self):
        p, S = self.plan(), self.nb_scores()
        out = [M.simulate(S[u], self.k, p, self.excl_of_user(u) if self.with_excl else None, self_id=self.nb_at() + u)
               for u in range(NU)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), [o[2] for o in out]


def _users(D, *pairs):
    """row users by (pattern, multiplier)"""
    return [PATTERNS.index(p) + D * MULTS.index(c) for p, c in pairs]


# Tall: many rows, one slice (or four), many rounds.  The + 5 leaves the last tile 5 rows.
TALL = [
    Case("tall_k128", "tall", 1500, 8, 128, 32768 + 5, 1, 12),
    Case("tall_k10_free", "tall", 1500, 9, 10, 32768 + 5, 1, 12, excl=False),
    Case("tall_k129", "tall", 1500, 9, 129, 16384 + 5, 1, 12),
    Case("tall_k256", "tall", 1500, 8, 256, 16384 + 5, 1, 12),
    Case("tall_k100_ragged", "tall", 1500, 8, 100, 8192 + 5, 4, 3),
    Case("tall_k100_specials", "tall", 1500, 9, 100, 8192 + 5, 4, 3, bi="specials", seed=1),
]

# Wide: a handful of rows, the most slices k allows, one item over a slice boundary: the last slice that holds candidates has a
# last round (or is a round) of one live candidate in wave 0, and the slices after it are empty.
WIDE = [
    Case("wide_k256", "wide", 24577, 8, 256, 37, 32, [7] * 27 + [4] + [0] * 4),
    Case("wide_k129", "wide", 48385, 9, 129, 37, 63, [7] * 54 + [1] + [0] * 8),
    Case("wide_k128", "wide", 24577, 8, 128, 37, 64, [4] * 48 + [1] + [0] * 15),
    Case("wide_k256_specials", "wide", 24579, 9, 256, 21, 32, [7] * 27 + [4] + [0] * 4, bi="specials", seed=2),
    Case("wide_k128_specials", "wide", 24578, 9, 128, 37, 64, [4] * 48 + [1] + [0] * 15, bi="specials", seed=3),
]

# Merge: three rows, a slice is one round (per = 128), up to the 256 lists the merge holds four to a lane.
MERGE = [
    Case("merge_64", "merge", 8192, 8, 32, 3, 64, 1,
         row_users=_users(8, ("spikes", 1.0), ("ascending", 1.0), ("spikes", 1.0))),
    Case("merge_65", "merge", 8193, 9, 7, 3, 65, 1,
         row_users=_users(9, ("ascending", 1.0), ("sawtooth", 1.0), ("ascending", 1.0))),
    Case("merge_129", "merge", 16385, 8, 32, 3, 129, 1,
         row_users=_users(8, ("plateaus", 1.0), ("spikes", -2.0), ("plateaus", 1.0))),
    Case("merge_193", "merge", 24577, 9, 20, 3, 193, 1,
         row_users=_users(9, ("scrambled", 1.0), ("ascending", 1.0), ("scrambled", 1.0))),
    Case("merge_256", "merge", 32768, 8, 32, 3, 256, 1,
         row_users=_users(8, ("spikes", 1.0), ("ascending", 1.0), ("spikes", 1.0))),
    Case("merge_256_constant", "merge", 32768, 8, 32, 3, 256, 1, bi="specials", seed=4,
         row_users=_users(8, ("constant", -1.0), ("sawtooth", 1.0), ("constant", -1.0))),
    Case("merge_256_half_empty", "merge", 32773, 9, 32, 3, 256, [2] * 128 + [1] + [0] * 127,
         row_users=_users(9, ("ascending", 1.0), ("spikes", 1.0), ("ascending", 1.0))),
    Case("merge_8_last_empty", "merge", 2500, 8, 129, 2048 + 5, 8, [3] * 6 + [2] + [0]),
]

CASES = TALL + WIDE + MERGE
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
