"""The logistic head stated once: sigmoid, its gradient, the cross-entropy and the rounded inference of one logit, in
NumPy ``longdouble``, with a first-order bound on what a float32 evaluation may lose of each.  NumPy only.

For a logit x (a float32 value, taken exactly) and a label z in {0, 1}:

  s     = 1 / (1 + exp(-x))
  g     = s - z, formed as -1 / (1 + exp(x)) for z = 1 so that the reference itself does not cancel
  l     = max(x, 0) - x z + log1p(exp(-|x|))
  infer = 0 for x <= 0 (both zeros), 1 for x >= 2^-20, unspecified in between

The tie rule is exact: e = exp(-x) >= 1 gives s = 1 / (1 + e) <= 0.5 in any monotone float32 evaluation, and half to even
takes 0.5 to 0; at x = 2^-20 sigmoid lies 2^-22 = four float32 spacings (2^-24 below 1) above 0.5 while the bound on the
head's s there is 1.5 spacings.  BPR's head is the z = 1 form on x = score(u, i) - score(u, j).

eps32 = 2^-24 is the unit throughout, as in tests/step_ref.py.  A device head is held to ``limit * eps32 * E``,
``limit = step_ref.limit_from`` of the ratio the float32 stand-in below reaches on the CPU - never of a device's."""
import numpy as np

LD = np.longdouble
F = np.float32
EPS32 = 2.0 ** -24
TINY = 2.0 ** -126                  # the smallest normal float32: a result below it may be flushed to zero
TIE = 2.0 ** -20                    # infer is specified outside (0, TIE)
LOG2E = F(1.4426950408889634)


def _ld(x):
    return np.asarray(np.asarray(x, F), LD)


def sigmoid(x):
    return 1 / (1 + np.exp(-_ld(x)))


def grad(x, z):
    x, z = _ld(x), np.asarray(z)
    with np.errstate(over="ignore"):
        return np.where(z == 1, -1 / (1 + np.exp(x)), 1 / (1 + np.exp(-x)))


def loss(x, z):
    x, z = _ld(x), np.asarray(z, LD)
    return np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x)))


def infer(x):
    """0, 1, or -1 where the rule leaves it open"""
    x = np.asarray(x, F)
    return np.where(x <= 0, 0, np.where(x >= F(TIE), 1, -1))


def E_g(x, z):
    """what float32 may lose of g, in units of eps32 (+ TINY absolute, see ``bound``)"""
    ax = np.abs(_ld(x))
    s, g = sigmoid(x), np.abs(grad(x, z))
    return np.asarray(
        s * (2                              # the sum 1 + e and the quotient 1 / (.) round once each: 2 eps32 relative to s
             + (ax + 2) * (1 - s))          # the exponential: __expf forms the float32-rounded product x * log2(e), off by
                                            # |x| eps32 relative in e (+ 2 for the product's constant and exp2 itself); a
                                            # relative error of e reaches s scaled by ds/dlog(e) = s (1 - s)
        + 2 * g,                            # the subtraction s - z rounds once; g is read back through m = fl(g (1 - b1))
        np.float64)


def E_l(x, z):
    """what float32 may lose of l, in units of eps32 (+ TINY absolute)"""
    x64, z = np.asarray(np.asarray(x, F), np.float64), np.asarray(z)
    ax = np.abs(_ld(x))
    sp = np.log1p(np.exp(-ax))
    return np.asarray(
        2 * ax * ((z == 1) | (x64 > 0))     # max(x, 0) - x z: the product (or its fused form) and the difference round at
                                            # magnitude |x| unless both terms are zero (z = 0 and x <= 0)
        + sp * (ax + 4)                     # the softplus log1p(e): e's relative error (|x| + 2, as above) reaches it at most
                                            # one to one (d log1p(e) / d log e = e / (1 + e) <= log1p(e) / e * e), log1p rounds
                                            # twice (its own evaluation and its result)
        + np.abs(loss(x, z)),               # the final addition rounds the result
        np.float64)


def E_l_sum(x, z):
    """the bound of a float32 sum of the B losses in any order: every partial sum rounds once, at most sum|l_k| each"""
    l = np.abs(np.asarray(loss(x, z), np.float64))
    return float(np.sum(E_l(x, z)) + (l.size - 1) * l.sum())


def E_g_sum(x, z):
    g = np.abs(np.asarray(grad(x, z), np.float64))
    return float(np.sum(E_g(x, z)) + (g.size - 1) * g.sum())


def bound(E):
    return EPS32 * np.asarray(E, np.float64) + TINY


def ratio(got, want, E):
    """max |got - want| / (eps32 E + TINY); inf where ``got`` is not finite"""
    got, want = np.atleast_1d(np.asarray(got, LD)), np.atleast_1d(np.asarray(want, LD))
    if got.size == 0:
        return 0.0
    if not np.isfinite(np.asarray(got, np.float64)).all():
        return float("inf")
    return float(np.max(np.abs(got - want) / np.asarray(bound(np.atleast_1d(E)), LD)))


def infer_wrong(got, x):
    """indices at which an inference contradicts the rule"""
    want = infer(x)
    return np.flatnonzero((want >= 0) & (np.asarray(got) != want))


# ----------------------------------------------------------------------------- the float32 stand-in
def _exp32(t, fast):
    """``fast``: __expf as exp2 of the float32-rounded product t * log2(e), the result rounded; else expf rounded
    correctly"""
    t = np.asarray(t, F)
    with np.errstate(over="ignore", under="ignore"):
        if fast:
            return np.exp2(np.asarray(t * LOG2E, np.float64)).astype(F)
        return np.exp(np.asarray(t, np.float64)).astype(F)


def standin(x, z, fast=True, mutant=None):
    """(g, l, infer) of the kernels' head (csrc/svd_kernels.h sigmoidf_, sigmoid_xent, binary_infer) with every operation
    rounded to float32.  ``mutant`` plants one of the heads the references must reject:

      "neglog"  l = -log(s) for z = 1, -log(1 - s) for z = 0
      "clamp"   s clamped to [1e-7, 1 - 1e-7]
      "oneminus"  g = 1 - sigmoid(-x) - z
      "floor"   infer = floor(s + 0.5)"""
    x, z = np.asarray(x, F), np.asarray(z, F)
    one = F(1)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        s = one / (one + _exp32(-x, fast))
        if mutant == "clamp":
            s = np.clip(s, F(1e-7), one - F(1e-7))
        g = s - z
        if mutant == "oneminus":
            g = (one - one / (one + _exp32(x, fast))) - z
        sp = np.log1p(np.asarray(_exp32(-np.abs(x), fast), np.float64)).astype(F)
        l = (np.maximum(x, F(0)) - x * z) + sp
        if mutant == "neglog":
            l = np.where(z == 1, -np.log(np.asarray(s, np.float64)), -np.log(np.asarray(one - s, np.float64))).astype(F)
        inf = np.floor(s + F(0.5)) if mutant == "floor" else np.rint(s)
    return g.astype(F), l.astype(F), inf.astype(F)


def sign0(q, mutant=False):
    """d|q|/dq as the steps use it under item_abs: sign(0) = 0 (``mutant``: sign(0) = 1)"""
    q = np.asarray(q)
    return np.where(q >= 0, 1.0, -1.0).astype(q.dtype) if mutant else np.sign(q)
