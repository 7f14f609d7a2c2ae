"""NumPy restatement of the reference's source / filter NMF and of
multiChanSourceF0Filter.initializeFreeMats (test infrastructure only).

`sfnmf_decomp_init` follows tools/nmf.py:161-360 line by line (the verbose
printing and plotting left out) and `initialize_free_mats`
audioModel.py:2878-2908, on oracle/fasst_ref.py's nmf_decomp_init and a
restatement model of tests/sf_ref.py (class_ref / RefFASSTsf, whose
renormalize_parameters is the reference's for several factors).
tests/golden/sfnmf.npz (runs of the reference,
tests/golden/make_golden_sfnmf.py) pins both (tests/test_sfnmf_ref_golden.py)."""
import numpy as np

eps = 10 ** -10     # nmf.py:22

# the golden cases of SFNMF_decomp_init (make_golden_sfnmf.py): the sizes, and
# per case the seed, which inits are supplied and the four switches
SFNMF_SHAPE = dict(F=65, N=47, K=13, Kf=6, Kr=2, niter=4)
SFNMF_CASES = {
    # name: (seed, inits supplied, (updateW, updateH, updateWFilt, updateHFilt))
    'free': (11, False, (True, True, True, True)),
    'inits': (12, True, (True, True, True, True)),
    'w_off': (13, True, (False, True, True, True)),
    'h_off': (14, True, (True, False, True, True)),
    'wfilt_off': (15, True, (True, True, False, True)),
    'hfilt_off': (16, True, (True, True, True, False)),
    'all_off': (17, True, (False, False, False, False)),
}
NAMES = ('W', 'H', 'WFilt', 'HFilt', 'Wres', 'Hres')


def case_inputs(name):
    """(SX, inits or None) of a golden case, from its own RandomState."""
    s = SFNMF_SHAPE
    seed, supplied, _ = SFNMF_CASES[name]
    rs = np.random.RandomState(1000 + seed)
    SX = np.dot(rs.randn(s['F'], 5) ** 2, rs.randn(5, s['N']) ** 2) + 1e-3
    inits = None
    if supplied:
        inits = dict(Winit=rs.randn(s['F'], s['K']) ** 2 + 1e-2,
                     Hinit=rs.randn(s['N'], s['K']) ** 2 + 1e-2,
                     WFiltInit=rs.randn(s['F'], s['Kf']) ** 2 + 1e-2,
                     HFiltInit=rs.randn(s['N'], s['Kf']) ** 2 + 1e-2)
    return SX, inits


def case_kwargs(name):
    s = SFNMF_SHAPE
    sw = SFNMF_CASES[name][2]
    return dict(nbComps=s['K'], nbFiltComps=s['Kf'], nbResComps=s['Kr'], niter=s['niter'],
                updateW=sw[0], updateH=sw[1], updateWFilt=sw[2], updateHFilt=sw[3])


def sfnmf_decomp_init(SX, nbComps=10, nbFiltComps=10, niter=10, Winit=None, Hinit=None,
                      WFiltInit=None, HFiltInit=None, updateW=True, updateH=True,
                      updateWFilt=True, updateHFilt=True, nbResComps=2):
    """tools/nmf.py:161-360"""
    freqs, nframes = SX.shape
    if Winit is None or (Winit.shape != (freqs, nbComps)):
        W = np.random.randn(freqs, nbComps) ** 2
    else:
        W = np.copy(Winit)
    if Hinit is None or (Hinit.shape != (nframes, nbComps)):
        H = np.random.randn(nframes, nbComps, ) ** 2
    else:
        H = np.copy(Hinit)
    if updateW:
        W /= W.sum(axis=0)
    if WFiltInit is None or (WFiltInit.shape != (freqs, nbFiltComps)):
        WFilt = np.random.randn(freqs, nbFiltComps) ** 2
    else:
        WFilt = np.copy(WFiltInit)
    if HFiltInit is None or (HFiltInit.shape != (nframes, nbFiltComps)):
        HFilt = np.random.randn(nframes, nbFiltComps, ) ** 2
    else:
        HFilt = np.copy(HFiltInit)
    if updateWFilt:
        WFilt /= WFilt.sum(axis=0)
    Wres = (1 + np.random.randn(freqs, nbResComps)) ** 2
    Hres = (1 + np.random.randn(nframes, nbResComps)) ** 2

    for i in range(niter):
        if updateW:
            SF0 = np.dot(W, H.T)
            SPHI = np.dot(WFilt, HFilt.T)
            Sres = np.dot(Wres, Hres.T)
            hatSX = SF0 * SPHI + Sres
            num = np.dot(SX * SPHI / np.maximum(hatSX ** 2, eps), H)
            den = np.dot(SPHI / np.maximum(hatSX, eps), H)
            W *= num / np.maximum(den, eps)
            sumW = W.sum(axis=0)
            sumW[sumW == 0] = 1.
            W /= sumW
            H *= sumW
        if updateH:
            SF0 = np.dot(H, W.T)
            SPHI = np.dot(HFilt, WFilt.T)
            Sres = np.dot(Hres, Wres.T)
            hatSX = SF0 * SPHI + Sres
            num = np.dot(SX.T * SPHI / np.maximum(hatSX ** 2, eps), W)
            den = np.dot(SPHI / np.maximum(hatSX, eps), W)
            H *= num / np.maximum(den, eps)
        if updateWFilt:
            SF0 = np.dot(W, H.T)
            SPHI = np.dot(WFilt, HFilt.T)
            Sres = np.dot(Wres, Hres.T)
            hatSX = SF0 * SPHI + Sres
            num = np.dot(SX * SF0 / np.maximum(hatSX ** 2, eps), HFilt)
            den = np.dot(SF0 / np.maximum(hatSX, eps), HFilt)
            WFilt *= num / np.maximum(den, eps)
            sumW = WFilt.sum(axis=0)
            sumW[sumW == 0] = 1.
            WFilt /= sumW
            HFilt *= sumW
        if updateHFilt:
            SF0 = np.dot(H, W.T)
            SPHI = np.dot(HFilt, WFilt.T)
            Sres = np.dot(Hres, Wres.T)
            hatSX = SF0 * SPHI + Sres
            num = np.dot(SX.T * SF0 / np.maximum(hatSX ** 2, eps), WFilt)
            den = np.dot(SF0 / np.maximum(hatSX, eps), WFilt)
            HFilt *= num / np.maximum(den, eps)
            # the sum goes into H before the zero guard (:316-319)
            sumH = HFilt.sum(axis=1)
            H *= np.vstack(sumH)
            sumH[sumH == 0] = 1.
            HFilt /= np.vstack(sumH)
        SF0 = np.dot(W, H.T)
        SPHI = np.dot(WFilt, HFilt.T)
        Sres = np.dot(Wres, Hres.T)
        hatSX = SF0 * SPHI + Sres
        num = np.dot(SX / np.maximum(hatSX ** 2, eps), Hres)
        den = np.dot(1 / np.maximum(hatSX, eps), Hres)
        Wres *= num / np.maximum(den, eps)
        sumW = Wres.sum(axis=0)
        sumW[sumW == 0] = 1.
        Wres /= sumW
        Hres *= sumW
        SF0 = np.dot(H, W.T)
        SPHI = np.dot(HFilt, WFilt.T)
        Sres = np.dot(Hres, Wres.T)
        hatSX = SF0 * SPHI + Sres
        num = np.dot(SX.T / np.maximum(hatSX ** 2, eps), Wres)
        den = np.dot(1 / np.maximum(hatSX, eps), Wres)
        Hres *= num / np.maximum(den, eps)
    return W, H.T, WFilt, HFilt.T, Wres, Hres


def mono_power(Cx):
    """audioModel.py:2883-2891 for two channels (Cx stored [c00, c01, c11])"""
    out = np.copy(np.real(Cx[0]))
    out += np.real(Cx[2])
    out /= np.double(2)
    return out


def initialize_free_mats(o, Cx, source_freq_comps, nb_comps, niter=10):
    """audioModel.py:2878-2908 on the restatement model `o` (tests/sf_ref.py
    class_ref): NMF on the fixed source dictionary, H shared out in place,
    the renormalisation."""
    nb_source = source_freq_comps.shape[1]
    import fasst_ref as R
    W, H = R.nmf_decomp_init(SX=mono_power(Cx),
                             Winit=np.dot(source_freq_comps,
                                          o.spec_comps[0]['factor'][0]['FW']),
                             nbComps=nb_source, niter=niter, updateW=False, updateH=True)
    for ncomp in range(nb_comps - 1):
        o.spec_comps[ncomp]['factor'][0]['TW'][:] = np.copy(H) / (nb_comps - 1)
    o.renormalize_parameters()


# ---- the class fixture of tests/golden/sfnmf.npz -------------------------------
CLASS_CFG = dict(F=33, T=21, nbComps=3, nbNMFResComps=2, nbFilterComps=6, nbFilterWeigs=[3, 3, 3],
                 spatial_rank=[1, 2, 1], nbSource=10, seed=3, niter=3)


def class_dicts():
    """Seeded small dictionaries and Cx for the object built without its
    constructor (as tests/test_sf_ref_golden.py does)."""
    c = CLASS_CFG
    rs = np.random.RandomState(4)
    F, T = c['F'], c['T']
    src = np.hstack([np.abs(rs.randn(F, c['nbSource'] - 1)) + 1e-3, np.ones((F, 1))])
    filt = np.abs(rs.randn(F, c['nbFilterComps'])) + 1e-3
    X = rs.randn(2, F, T) + 1j * rs.randn(2, F, T)
    Cx = np.array([np.abs(X[0]) ** 2, X[0] * np.conj(X[1]), np.abs(X[1]) ** 2])
    return src, np.eye(c['nbSource']), filt, Cx


def bare_model(cls, src, srcw, filt, Cx):
    """An instance of `cls` (the reference's or the product's
    multiChanSourceF0Filter) with the attributes its _initialize_structures
    and initializeFreeMats read, set by hand."""
    c = CLASS_CFG

    class Audio(object):
        channels = 2
    m = object.__new__(cls)
    m.audioObject, m.verbose, m.sparsity = Audio(), 0, None
    m.nbFreqsSigRepr, m.nbFramesSigRepr = c['F'], c['T']
    m.nbComps, m.nbNMFResComps = c['nbComps'], c['nbNMFResComps']
    m.nbFilterComps, m.nbFilterWeigs = c['nbFilterComps'], list(c['nbFilterWeigs'])
    m.spatial_rank = list(c['spatial_rank'])
    m.sourceFreqComps, m.sourceFreqWeights, m.filterFreqComps = src, srcw, filt
    m.nbSourceComps = src.shape[1]
    m.iter_num = 2
    if isinstance(getattr(cls, 'Cx', None), property):
        # the product's Cx setter opens a device engine: set the host copy
        m._engine, m.device, m._Cx = None, None, np.asarray(Cx, dtype=np.complex128)
    else:
        m.Cx = Cx
    return m
