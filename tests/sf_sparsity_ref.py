"""NumPy restatement of multiChanSourceF0Filter.reweigh_sparsity_constraint
(audioModel.py:2981-3014) and of the sigma schedule of its
estim_param_a_post_model (:2939-2977), written to run on the restatement's
model (tests/sf_ref.py RefFASSTsf) or any model with the reference's dict
layout.  Test infrastructure only.

`dtype` selects the arithmetic of the barycentre and of the mask: float64 is
the reference's; np.longdouble gives the figure the GPU tests' tolerance is
measured against (tests/test_gpu_sf_sparsity.py)."""
import numpy as np

EPS = 1e-10

# the sf_sparse fixture (tests/golden/make_golden_sf_sparsity.py): the sf_inst
# model with these per-component sparsity lengths
SPARSE_CASE = 'sf_inst'
SPARSE_LENGTHS = [3, False, 2]


def median_filter(x, length):
    """tools/signalTools.py:13-24"""
    N = x.size
    out = np.zeros_like(x)
    for n in range(N):
        w = x[max(n - length, 0):min(n + length, N - 1)]
        out[n] = np.median(w) if w.size else np.nan
        if np.isnan(out[n]):
            out[n] = x[n]
    return out


def barycentre(TW, dtype=np.float64):
    """:2994-3000: the energy barycentre of every column over the rows but the
    last one."""
    K = TW.shape[0]
    TW = TW.astype(dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        return (np.dot((np.arange(K - 1) * (np.arange(K - 1, 0, -1)) ** 2).astype(dtype), TW[:-1, :]) /
                np.dot(((np.arange(K - 1, 0, -1)) ** 2).astype(dtype),
                       np.maximum(TW[:-1, :], dtype(EPS))))


def mask(mu, K, sigma, dtype=np.float64):
    """:3007-3013: the Gaussian mask around the track, its last row the column
    maximum, normalised where that maximum is > 0."""
    mu = mu.astype(dtype)
    with np.errstate(invalid='ignore', under='ignore'):
        m = np.exp(dtype(-0.5) * ((np.vstack(np.arange(K)).astype(dtype) - mu) ** 2) / dtype(sigma))
        m[-1] = m.max(axis=0)
        m[:, m[-1] > 0] /= m[-1][m[-1] > 0]
    return m


def reweigh_tw(TW, length, sigma, dtype=np.float64):
    """The body of the loop (:2991-3014) on one TW, in place; returns (the
    filtered track, the mask)."""
    mu = median_filter(barycentre(TW, dtype), length)
    m = mask(mu, TW.shape[0], sigma, dtype)
    with np.errstate(invalid='ignore'):
        TW *= m.astype(TW.dtype)
    return mu, m


def reweigh_sparsity_constraint(model, sigma, nbComps=None):
    """:2987-3014 on a model's dicts; nbComps defaults to every spectral
    component (the class keeps nbComps == len(spec_comps))."""
    n = len(model.spec_comps) if nbComps is None else nbComps
    for j in range(n):
        comp = model.spec_comps[j]
        if comp.get('sparsity') and comp['factor'][0]['TW'].shape[0] > 2:
            reweigh_tw(comp['factor'][0]['TW'], comp['sparsity'], sigma)


def sigma_schedule(model, iter_num=None):
    """:2939-2941, 2973-2976: from K^2 (K the largest factor-0 TW.shape[0] over
    ALL spectral components) to 9, geometrically."""
    n = model.iter_num if iter_num is None else iter_num
    logSigma0 = np.log(np.max([spec['factor'][0]['TW'].shape[0]
                               for spec in model.spec_comps.values()]) ** 2)
    logSigmaInf = np.log(9.0)
    return np.array([np.exp(logSigma0 + (logSigmaInf - logSigma0) / max(n - 1.0, 1.) * i)
                     for i in range(n)])


def estim_param_a_post_model(model, after=None):
    """:2933-2979 on the restatement: its own iterations, each followed by the
    reweighting at the schedule's sigma."""
    sig = sigma_schedule(model)

    def step(i, mod):
        reweigh_sparsity_constraint(mod, sig[i])
        if after is not None:
            after(i, mod)
    return model.estim_param_a_post_model(callback=step)


# ---- the bare-reweigh cases of tests/test_gpu_sf_sparsity.py: (K, T, L) ----
BARE_SHAPES = [
    (3, 300, 3),      # smallest K; T no multiple of a frame chunk
    (14, 300, 150),   # halo wider than a chunk
    (14, 40, 64),     # window clipped on both sides, L >= T
    (14, 2, 3),       # the only window holds one sample
    (14, 1, 3),       # empty window: the sample itself
    (2, 50, 3),       # K <= 2: skipped
    (129, 257, 10),   # past 128 rows, T one over a chunk
    (300, 130, 10),   # past the Python layer's cap (engine level)
]


# precision_gap() as measured (tests/test_sf_sparsity_ref_golden.py keeps it
# current), and the GPU tests' bound on a reweighed TW: 16 x the gap, floor
# 1e-13.  The margin covers the device's own summation order in the barycentre
# and an exp within 1-2 ulp
PRECISION_GAP = 1.512e-14
REWEIGH_TOL = max(16 * PRECISION_GAP, 1e-13)


def bare_sigmas(K):
    return (float(K) ** 2, 9.0)


def bare_tw(K, T, zero_col=None):
    """Seeded positive random TW; zero_col: that column all zero."""
    TW = 0.75 * np.abs(np.random.RandomState(1000 * K + T).randn(K, T)) + 0.25
    if zero_col is not None:
        TW[:, zero_col] = 0.0
    return TW


def precision_gap(shapes=BARE_SHAPES):
    """The largest relative gap (max |a - b| / max |b|) between the float64
    and the np.longdouble evaluation of the filtered track and of the mask
    over the bare cases: what float64 arithmetic alone costs here."""
    worst = 0.0
    for K, T, L in shapes:
        if K <= 2:
            continue
        for zero_col in (None, T // 2):
            for sigma in bare_sigmas(K):
                TW = bare_tw(K, T, zero_col)
                mu, m = reweigh_tw(TW.copy(), L, sigma)
                mul, ml = reweigh_tw(TW.astype(np.longdouble), L, sigma, np.longdouble)
                for a, b in ((mu, mul), (m, ml)):
                    den = float(np.max(np.abs(b))) or 1.0
                    worst = max(worst, float(np.max(np.abs(a - b))) / den)
    return worst


def set_sparsity(model, lengths=SPARSE_LENGTHS):
    for j, L in enumerate(lengths):
        model.spec_comps[j]['sparsity'] = L
