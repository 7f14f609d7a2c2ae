"""NumPy restatement of the reference's discrete-state time weights
(TW_constr 'GSMM' / 'SHMM', audioModel.py:1728-1928) on top of the oracle
model of oracle/fasst_ref.py, and the hmm_* fixture helpers.

RefFASST restates the NMF branch only; RefFASSTConstr overrides
update_spectral_components with the constrained branch, quirks included:
  * the Viterbi accumulates (`accumulateVec += tmp[ante] + ISdiv`, :1868-1872)
    where a textbook Viterbi assigns;
  * backtracking reads antecedentMat[state[n], n - 1] (:1881-1885), column
    n - 1 rather than n, so column 0 (never written, zeros) decides frame 0;
  * TW_all persists in the factor and renormalize_parameters never scales it;
  * 'GMM' / 'HMM' raise from renormalize_parameters (:2015,2038-2040), after
    the update has already moved the model.
Every argmin goes through _argmin, which records the smallest gap between
the best and second-best candidate relative to max(|best|, 1) (self.margin):
the tests require it to be >= MARGIN_MIN so that no decision rests on
rounding.
"""
import json
import warnings

import numpy as np

import fasst_ref as R

EPS = R.EPS
MARGIN_MIN = 1e-6


def argmin_margin(x, axis=None):
    """Smallest (second best - best) / max(|best|, 1) over the argmins of x."""
    x = np.asarray(x, dtype=float)
    if x.ndim == 1 or axis is None:
        x = x.reshape(-1, 1)
        axis = 0
    if x.shape[axis] < 2:
        return np.inf
    s = np.sort(x, axis=axis)
    best, second = np.take(s, 0, axis=axis), np.take(s, 1, axis=axis)
    return float(np.min((second - best) / np.maximum(np.abs(best), 1.)))


class RefFASSTConstr(R.RefFASST):
    def __init__(self, *a, **kw):
        super(RefFASSTConstr, self).__init__(*a, **kw)
        self.margin = np.inf
        self.state_seqs = []     # per update_spectral_components call: {spec key: states}

    def _argmin(self, x, axis=None):
        self.margin = min(self.margin, argmin_margin(x, axis))
        return np.argmin(x, axis=axis)

    # audioModel.py:1469-1978 with the discrete-state branch (:1728-1928)
    def update_spectral_components(self, hat_W):
        held = []
        for k, comp in self.spec_comps.items():
            for fi, fac in comp['factor'].items():
                if fac['TW_frdm_prior'] == 'free' and fac['TW_constr'] != 'NMF':
                    if fac['TW_constr'] not in ('GMM', 'GSMM', 'HMM', 'SHMM'):
                        raise NotImplementedError("TW_constr %s" % fac['TW_constr'])
                    if self.lambdaCorr > 0 or len(comp['factor']) > 1 or \
                            sum(c['spat_comp_ind'] == comp['spat_comp_ind']
                                for c in self.spec_comps.values()) > 1:
                        # the order of the per-component updates would matter
                        raise NotImplementedError("restated for a constrained component alone "
                                                  "on its spatial component, lambdaCorr = 0")
                    held.append((k, comp, fac))
                    fac['TW_frdm_prior'] = 'fixed'
        try:   # FB / FW of every component, TW of the NMF ones
            super(RefFASSTConstr, self).update_spectral_components(hat_W)
        finally:
            for k, comp, fac in held:
                fac['TW_frdm_prior'] = 'free'
        seqs = {}
        for k, comp, fac in held:
            seqs[k] = self._update_tw_constrained(k, comp, fac, hat_W)
        self.state_seqs.append(seqs)

    def _update_tw_constrained(self, k, comp, fac, hat_W):
        omega = self.nmfUpdateCoeff
        j = comp['spat_comp_ind']
        T = self.nbFramesSigRepr
        warnings.warn("The GMM/GSMM/HMM still needs to be adapted " +
                      "to take into account the different factors. ")          # :1729-1731
        nb = fac['TW'].shape[0]
        if len(fac['TB']):                                                     # :1736-1742
            raise AttributeError("In this implementation, as in Ozerov's, non-trivial time "
                                 "blobs TB is incompatible with discrete state-based "
                                 "constraints for the time weights TW")
        if 'TW_all' not in fac:                                                # :1744-1748
            fac['TW_all'] = np.outer(np.ones(nb), np.max(fac['TW'], axis=0))
        if 'TW_DP_params' not in fac:                                          # :1750-1760
            if fac['TW_constr'] in ('GMM', 'GSMM'):
                fac['TW_DP_params'] = np.ones(nb) / np.double(nb)
            else:
                fac['TW_DP_params'] = np.ones([nb, nb]) / np.double(nb)
        if fac['TW_constr'] in ('GMM', 'HMM') and \
                (np.max(fac['TW_all']) > 1 or np.min(fac['TW_all']) < 1):       # :1762-1766
            fac['FB'] *= np.mean(fac['TW_all'])
            fac['TW_all'][:] = 1.
        IS = np.zeros([nb, T])
        for c in range(nb):                                                    # :1773-1832
            fac['TW'][:] = 0
            fac['TW'][c] = fac['TW_all'][c]
            if fac['TW_constr'] not in ('GMM', 'HMM'):
                V = np.maximum(self.comp_spat_comp_power(j, spec_comp_ind=[k]), EPS)
                Wb = np.dot(fac['FB'], fac['FW'][:, c])
                num = np.dot(Wb, hat_W[j] / np.maximum(V ** 2, EPS))
                den = np.dot(Wb, 1 / V)
                fac['TW'][c] *= (num / np.maximum(den, EPS)) ** omega
                fac['TW_all'][c] = fac['TW'][c]
            P = np.maximum(self.comp_spat_comp_power(j), EPS)
            r = hat_W[j] / P
            IS[c] = np.sum(r - np.log(np.maximum(r, EPS)) - 1, axis=0)
        self.last_ISdiv = IS.copy()
        if fac['TW_constr'] in ('GMM', 'GSMM'):                                # :1840-1847
            seq = self._argmin(IS - np.vstack(np.log(fac['TW_DP_params'] + EPS)), axis=0)
        else:                                                                  # :1853-1885
            acc = IS[:, 0] - np.log(1. / nb)
            ante = np.zeros([nb, T], dtype=np.int32)
            for n in range(1, T):
                tmp = np.vstack(acc) - np.log(fac['TW_DP_params'] + EPS)
                ante[:, n] = self._argmin(tmp, axis=0)
                acc += tmp[ante[:, n], range(nb)] + IS[:, n]
                acc -= acc.min()
            seq = np.zeros(T, dtype=np.int32)
            seq[-1] = self._argmin(acc)
            for n in range(T - 1, 0, -1):
                seq[n - 1] = ante[seq[n], n - 1]
        fac['TW'][:] = 0.                                                      # :1895-1900
        for n in range(T):
            fac['TW'][seq[n], n] = fac['TW_all'][seq[n], n]
        if fac['TW_DP_frdm_prior'] == 'free':                                  # :1902-1924
            if fac['TW_constr'] in ('GMM', 'GSMM'):
                for c in range(nb):
                    fac['TW_DP_params'][c] = np.sum(seq == c) * 1. / T
            else:
                for p in range(nb):
                    den = np.sum(seq[:-1] == p)
                    if den:
                        for q in range(nb):
                            num = 1. * np.sum((seq[:-1] == p) * (seq[1:] == q))
                            fac['TW_DP_params'][p, q] = num / den
        return np.array(seq, dtype=np.int32)


# audioModel.py:2534-2549
def make_shmm(model):
    for comp in model.spec_comps.values():
        for fac in comp['factor'].values():
            nb = fac['TW'].shape[0]
            fac['TW_constr'] = 'SHMM'
            fac['TW_DP_params'] = 9 * np.eye(nb)
            fac['TW_DP_params'] += 1.
            fac['TW_DP_params'] /= np.vstack(fac['TW_DP_params'].sum(axis=1))
            fac['TW_DP_frdm_prior'] = 'fixed'


def constrain(model, kind, keys=None, dp_free=False):
    """TW_constr = kind on the spectral components `keys` (default: all) of a
    product, reference or oracle model; the prior is left to its first-use
    default."""
    for k in (sorted(model.spec_comps) if keys is None else keys):
        fac = model.spec_comps[k]['factor'][0]
        fac['TW_constr'] = kind
        fac['TW_DP_frdm_prior'] = 'free' if dp_free else 'fixed'


# tests/golden/hmm_<case>.npz: the structure applied after makeItConvolutive
HMM_CASES = {
    "hmm_shmm": lambda m: m.makeItSHMM() if hasattr(m, 'makeItSHMM') else make_shmm(m),
    "hmm_shmm_free": lambda m: constrain(m, 'SHMM', dp_free=True),
    "hmm_gsmm": lambda m: constrain(m, 'GSMM', dp_free=True),
}


def oracle_from_fixture(g, case):
    """RefFASSTConstr on the fixture's WAV, initialised as the reference was."""
    ctor = json.loads(str(g['ctor']))
    kw = ctor['kw']
    x, _ = R.read_scaled(g['wav'])
    w = np.hanning(kw['wlen'])
    X = [R.stft(x[:, c], w, kw['hopsize'], kw['wlen']) for c in range(2)]
    m = RefFASSTConstr(iter_num=kw['iter_num'])
    m.set_transform(X)
    np.random.seed(0)
    R.init_nmf_inst(m, ctor['nbComps'], ctor['nbNMFComps'], ctor['spatial_rank'])
    R.make_convolutive(m)
    HMM_CASES[case](m)
    return m
