"""NumPy restatement of the reference's stereo_NMF
(SeparateLeadStereo/SIMM/SIMM.py:945-1104), line by line, with the
reconstruction error vector returned as well (the reference computes it and
drops it).  Pinned bit for bit to the reference's own outputs by
tests/test_stereo_nmf_ref_golden.py (fixture tests/golden/stereo_nmf.npz,
written by tests/golden/make_golden_stereo_nmf.py).

Also the golden cases' inputs, shared by the generator and the tests.
"""
import numpy as np
from numpy.random import randn

EPS = 10 ** (-20)
NAMES = ("betaR", "betaL", "HM", "WM")

# case -> (seed, F, N, R, iterations, omega, which inits are supplied)
CASES = {
    "rand": (11, 65, 22, 5, 5, 1.0, None),
    "given": (12, 47, 19, 4, 4, 1.0, "given"),
    "omega07": (13, 33, 17, 3, 5, 0.7, None),
    "wrongshape": (14, 40, 18, 4, 3, 1.0, "wrongshape"),
    "r1": (15, 33, 25, 1, 4, 1.0, None),
}


def ISDistortion(X, Y):
    """tools/distances.py:9-17"""
    return np.sum((-np.log(X / Y) + (X / Y) - 1))


def make_data(seed, F, N, R=4):
    """Two positive planes that share a low-rank structure with different
    panning, plus a noise floor (its own generator: the global stream is the
    function's)."""
    rng = np.random.RandomState(1000 + seed)
    W = np.abs(rng.randn(F, R + 1)) ** 2
    H = np.abs(rng.randn(R + 1, N)) ** 2
    b = rng.rand(R + 1)
    SXR = np.dot(W * b ** 2, H) + 1e-3 * rng.rand(F, N)
    SXL = np.dot(W * (1 - b) ** 2, H) + 1e-3 * rng.rand(F, N)
    return SXR, SXL


def case_inputs(name):
    """(SXR, SXL, kwargs of stereo_NMF besides the data, seed)"""
    seed, F, N, R, niter, omega, inits = CASES[name]
    SXR, SXL = make_data(seed, F, N)
    kw = dict(numberOfAccompanimentSpectralShapes=R, numberOfIterations=niter,
              updateRulePower=omega)
    rng = np.random.RandomState(2000 + seed)
    if inits == "given":
        kw["WM0"] = np.abs(rng.randn(F, R)) + 0.1
        kw["HM0"] = np.abs(rng.randn(R, N)) + 0.1
    elif inits == "wrongshape":
        kw["WM0"] = np.abs(rng.randn(F + 1, R)) + 0.1
    return SXR, SXL, kw, seed


def initial_draw(F, N, R, WM0=None, HM0=None):
    """SIMM.py:968-991: HM0, then WM0, then betaR from the global stream; a
    matrix is drawn when it is not given or has the wrong shape."""
    def pick(given, shape):
        if given is not None:
            g = np.array(given)
            if g.shape[0] == shape[0] and g.shape[1] == shape[1]:
                return np.copy(g)
        return np.abs(randn(*shape))
    HM = pick(HM0, (R, N))
    WM = pick(WM0, (F, R))
    betaR = np.diag(np.random.rand(R))
    return WM, HM, betaR


def _model(WM, HM, beta):
    # :993-994 and after every step: the product order is (WM beta^2) HM
    return np.maximum(np.dot(np.dot(WM, beta ** 2), HM), EPS)


def _ratios(SX, hat):
    # the two clamps: hat itself (inside _model) and hat ** 2 again
    return SX / np.maximum(hat ** 2, EPS), 1 / np.maximum(hat, EPS)


def iterate(SXR, SXL, WM, HM, betaR, numberOfIterations, omega):
    """SIMM.py:991-1104 from a given starting point (betaR a diagonal
    matrix), every floating-point operation in the reference's order."""
    F, N = SXR.shape
    R = WM.shape[1]
    betaL = np.eye(R) - betaR
    reco = np.zeros([numberOfIterations * 3 + 1])
    k = [0]

    def model_and_error():
        hR, hL = _model(WM, HM, betaR), _model(WM, HM, betaL)
        reco[k[0]] = ISDistortion(SXR, hR) + ISDistortion(SXL, hL)
        k[0] += 1
        return hR, hL

    hatR, hatL = model_and_error()
    for _ in np.arange(numberOfIterations):
        # HM step (:1021-1031): denominator clamped
        pR, qR = _ratios(SXR, hatR)
        pL, qL = _ratios(SXL, hatL)
        gR, gL = np.dot(betaR ** 2, WM.T), np.dot(betaL ** 2, WM.T)
        HM = HM * ((np.dot(gR, pR) + np.dot(gL, pL)) /
                   np.maximum(np.dot(gR, qR) + np.dot(gL, qL), EPS)) ** omega
        hatR, hatL = model_and_error()

        # WM step (:1045-1060): denominator not clamped, then the column sums
        pR, qR = _ratios(SXR, hatR)
        pL, qL = _ratios(SXL, hatL)
        gR, gL = np.dot(HM.T, betaR ** 2), np.dot(HM.T, betaL ** 2)
        WM = WM * ((np.dot(pR, gR) + np.dot(pL, gL)) /
                   (np.dot(qR, gR) + np.dot(qL, gL))) ** omega
        sumWM = np.sum(WM, axis=0)
        pos = sumWM > 0
        WM[:, pos] = WM[:, pos] / np.outer(np.ones(F), sumWM[pos])
        HM = HM * np.outer(sumWM, np.ones(N))
        hatR, hatL = model_and_error()

        # beta step (:1075-1090): only the diagonal of the R x R ratio survives
        pR, qR = _ratios(SXR, hatR)
        pL, qL = _ratios(SXL, hatL)
        with np.errstate(all='ignore'):     # off-diagonal 0 * inf of the full matrices
            betaR = np.diag(np.diag(np.maximum(
                betaR * (np.dot(np.dot(WM.T, pR), HM.T) /
                         np.dot(np.dot(WM.T, qR), HM.T)) ** (omega * .1), EPS)))
            betaL = np.diag(np.diag(np.maximum(
                betaL * (np.dot(np.dot(WM.T, pL), HM.T) /
                         np.dot(np.dot(WM.T, qL), HM.T)) ** (omega * .1), EPS)))
        betaR = betaR / np.maximum(betaR + betaL, EPS)
        betaL = np.copy(np.eye(R) - betaR)
        hatR, hatL = model_and_error()
    return betaR, betaL, HM, WM, reco


def stereo_NMF(SXR, SXL, numberOfAccompanimentSpectralShapes, WM0=None, HM0=None,
               numberOfIterations=50, updateRulePower=1.0):
    """(betaR, betaL, HM, WM, reco_error); draws from the global stream"""
    R = numberOfAccompanimentSpectralShapes
    F, N = SXR.shape
    if (F, N) != SXL.shape:
        raise ValueError("Dimension of STFT matrices must be the same.")
    WM, HM, betaR = initial_draw(F, N, R, WM0, HM0)
    return iterate(SXR, SXL, WM, HM, betaR, numberOfIterations, updateRulePower)
