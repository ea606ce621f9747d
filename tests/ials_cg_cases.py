"""Cases for the conjugate-gradient half-sweeps of the implicit ALS (tests/test_ials_cg_ref_host.py,
tests/test_gpu_ials_cg.py): the dict format and the generators are those of tests/ials_cases.py.

Every case comes with two sets of tables: its own, uniform in [0, 1), and ``normal(case)``, drawn N(0, 0.1) (signs cancel in
the list sums and in G v, and the warm start is far from the minimiser's scale).  CASES holds both orientations of both.
"""
import numpy as np

from tests import ials_cases as C

# both ends of every count of components per lane, ceil(d / 64) = 1 .. 4 (csrc/ials_cg.hip cg_pass), one past 64 and 128,
# and d = 1
WIDTHS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
# one entity per length.  Entry k goes to wave k mod 4: up to 3 entries some waves have none, around 4 and 8 their shares
# become unequal.  A wave gathers four of its entries ahead (CG_AHEAD, 16 list entries per round of the block): at 12 no
# wave has a full round, at 13 wave 0 alone has one, at 16 all four have one and nothing after it, at 17 wave 0 has a round
# and a single entry after it; 31 .. 65 lie around two and four rounds
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 31, 32, 33, 63, 64, 65)
LONG_LENGTHS = C.LONG_LENGTHS + (1100,)                    # 1100: every partner, the longest sum of the suite
LONG_WIDTHS = (1, 65, 256)
# the Gram of both solvers: both ends of every count of 64-wide output tiles per side, 1 .. 4, and the widths around them; a
# thread's 4 x 4 block partly or wholly past d and a partly filled single tile (17, 33); both sides of the width below which
# the narrow kernel takes over (23, 24), and small widths of that kernel (1 slot: 3, 4, 5; 2: 17; 3: 23)
GRAM_WIDTHS = (1, 3, 4, 5, 17, 23, 24, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)
GRAM_NS = (1, 127, 128, 129, 5 * 128 + 3)                  # 131 073 rows (slices of 160) run at d = 65 only
LAMBDAS = (0.1, 1e-3, 1e-6)
ALPHAS = (1.0, 40.0)
CONV_WIDTHS = (1, 9, 33)                                   # cg_steps = 3 d against the exact minimiser
STEPS = (1, 2, 3)


def widths_case(d):
    """one user per list length over 80 items; two further users without pairs"""
    rs = np.random.RandomState(7000 + d)
    return C._case("cg-widths-d%d" % d, d, 0.1, 40.0, 512, len(LENGTHS) + 2, 80, C._of_lengths(rs, LENGTHS, 80), rs)


def long_case(d):
    """lists of 511 .. 1025 and of all 1100 partners, a short one and an empty one"""
    rs = np.random.RandomState(7500 + d)
    lengths = LONG_LENGTHS + (40, 0)
    return C._case("cg-long-d%d" % d, d, 0.1, 40.0, 512, len(lengths), 1100, C._of_lengths(rs, lengths, 1100), rs)


def conditioning(lam, alpha):
    """d = 256 with 1, 5 and 40 pairs (far fewer than components: only G and the ridge make A definite), 300 pairs and none"""
    rs = np.random.RandomState(7900)
    return C._case("cg-conditioning-lam%g-alpha%g" % (lam, alpha), 256, lam, alpha, 512, 5, 320,
                   C._of_lengths(rs, (1, 5, 40, 300, 0), 320), rs)


def normal(c, seed=1):
    """the same data with both tables drawn N(0, 0.1)"""
    rs = np.random.RandomState(seed + 31 * c["d"] + c["nu"])
    return dict(c, id=c["id"] + "-normal", X=rs.normal(0.0, 0.1, c["X"].shape), Y=rs.normal(0.0, 0.1, c["Y"].shape))


def _all_forms(cases):
    """as given and swapped, each with its uniform tables and with normal ones"""
    return [f for c in C.both(cases) for f in (c, normal(c))]


CASES = _all_forms([widths_case(d) for d in WIDTHS] + [long_case(d) for d in LONG_WIDTHS])
CONV_CASES = _all_forms([dict(widths_case(d), id="cg-conv-d%d" % d) for d in CONV_WIDTHS])
CONDITIONING = [conditioning(lam, alpha) for lam in LAMBDAS for alpha in ALPHAS]
# the cases whose loss is restated on the CPU: one per count of components per lane, and d = 1
LOSS_IDS = tuple(c["id"] for c in CASES if c["id"].startswith("cg-widths") and c["d"] in (1, 65, 128, 256))
