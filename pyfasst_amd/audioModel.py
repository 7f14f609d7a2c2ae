"""FASST model classes with the reference's surface, running on MI355X.

Drop-in for pyfasst.audioModel (audioModel.py:66-2508): same class names,
constructor keyword arguments, `spat_comps` / `spec_comps` / `noise` dicts
and public methods.  Between calls the NumPy dicts are the source of truth;
`estim_param_a_post_model()` uploads them once, runs every GEM iteration on
the GPU (pyfasst_amd/csrc/fasst_em.hip and its phase units fasst_em_*.hip) and downloads the result;
`separate_spat_comps()` computes the Wiener images and iSTFTs on the GPU.

There is no CPU fallback: structures outside the HIP path raise
NotImplementedError, a missing library raises ImportError.

Deliberate deviation: the reference stores the shared
mutable default `ann_PSD_lim=[None, None]` by reference, so a second model
in the same process inherits the first model's annealing limits
(audioModel.py:166,242,320-323); here each model copies the list.
"""
import os
import warnings

import numpy as np

from . import audioObject as ao
from .engine import Engine
from .tftransforms import minqt as minqt_mod
from .tftransforms import stft as stft_mod

eps = 1e-10              # audioModel.py:61
log_prior_small_cst = 1e-70
soundCelerity = 340.


class FASST(object):
    """FASST base class (audioModel.py:66-248)."""
    implemented_transf = ['stft', 'mqt', 'minqt', 'cqt']
    implemented_annealing = ['ann', 'no_ann']

    def __init__(self, audio, transf='stft', wlen=2048, hopsize=512, iter_num=50,
                 sim_ann_opt='ann', ann_PSD_lim=[None, None], verbose=0, nmfUpdateCoeff=1.,
                 tffmin=25, tffmax=18000, tfWinFunc=None, tfbpo=48, lambdaCorr=0.,
                 device=None):
        self.verbose = verbose
        self.nmfUpdateCoeff = nmfUpdateCoeff
        if isinstance(audio, ao.AudioObject):
            self.audioObject = audio
        elif isinstance(audio, str):
            self.audioObject = ao.AudioObject(filename=audio)
        else:
            raise AttributeError("The provided audio parameter is" + "not a supported format.")
        self.device = device
        self.sig_repr_params = {}
        self.sig_repr_params['transf'] = transf.lower()
        self.sig_repr_params['wlen'] = ao.nextpow2(wlen)
        self.sig_repr_params['fsize'] = ao.nextpow2(wlen)
        self.sig_repr_params['hopsize'] = hopsize
        self.sig_repr_params['tffmin'] = tffmin
        self.sig_repr_params['tffmax'] = tffmax
        self.sig_repr_params['tfbpo'] = tfbpo
        self.sig_repr_params['tfWinFunc'] = tfWinFunc
        self.sig_repr_params['hopfactor'] = 1. * hopsize / self.sig_repr_params['wlen']
        if self.sig_repr_params['transf'] not in self.implemented_transf:
            raise NotImplementedError(self.sig_repr_params['transf'] + " not yet implemented.")
        # the transform object (audioModel.py:205-214): STFT, or the rasterised
        # MinQT / CQT (perfRast=1) on the GPU
        tf_cls = {'stft': stft_mod.STFT, 'mqt': minqt_mod.MinQTransfo,
                  'minqt': minqt_mod.MinQTransfo, 'cqt': minqt_mod.CQTransfo}[
                      self.sig_repr_params['transf']]
        self.tft = tf_cls(fmin=tffmin, fmax=tffmax, bins=tfbpo, fs=self._samplerate_or_default(),
                          perfRast=1, linFTLen=self.sig_repr_params['fsize'],
                          atomHopFactor=self.sig_repr_params['hopfactor'], device=device)
        self.demixParams = {
            'tffmin': tffmin, 'tffmax': tffmax, 'tfbpo': tfbpo,
            'tfrepresentation': transf.lower(), 'wlen': self.sig_repr_params['wlen'],
            'hopsize': self.sig_repr_params['wlen'] // 2, 'neighbors': 20, 'winFunc': tfWinFunc}
        self.noise = {}
        self.noise['PSD'] = np.zeros(self.sig_repr_params['fsize'] // 2 + 1)
        self.noise['sim_ann_opt'] = sim_ann_opt
        self.noise['ann_PSD_lim'] = list(ann_PSD_lim)
        self.spat_comps = {}
        self.spec_comps = {}
        self.iter_num = iter_num
        self.lambdaCorr = lambdaCorr
        self._engine = None
        self._Cx = None

    def _samplerate_or_default(self):
        try:
            return self.audioObject.samplerate
        except Exception:
            return 44100

    # ---------------------------------------------------------------- Cx
    @property
    def Cx(self):
        """Packed covariance [3, F, T] (audioModel.py:293-302), fetched lazily."""
        if self._Cx is None and self._engine is not None:
            self._Cx = self._engine.get_cx()
        return self._Cx

    @Cx.setter
    def Cx(self, value):
        value = np.asarray(value, dtype=np.complex128)
        self._Cx = value
        if value.ndim == 3:
            self.nbFreqsSigRepr, self.nbFramesSigRepr = value.shape[1:]
            if (self._engine is None or self._engine.F != value.shape[1]
                    or self._engine.T != value.shape[2]):
                self._engine = Engine(value.shape[1], value.shape[2], self.device)
            self._engine.set_cx(value)

    def comp_transf_Cx(self):
        """Signal representation on the GPU (audioModel.py:250-328)."""
        if self.sig_repr_params['transf'] not in self.implemented_transf:
            raise ValueError(self.sig_repr_params['transf'] + " not implemented - yet?")
        aud = self.audioObject
        if isinstance(aud, ao.SpectralAudio):
            F, T = aud.nbFreqs, aud.nbFrames
            self._engine = Engine(F, T, self.device)
            self.nbFreqsSigRepr, self.nbFramesSigRepr = F, T
            if aud.X is not None:
                self._engine.set_stft(aud.X)   # Cx packed on the device
                self._Cx = None
            else:
                self.Cx = aud.Cx
        else:
            if not hasattr(aud, '_data'):
                aud._read()
            nc = aud.channels
            if nc != 2:
                raise NotImplementedError("the HIP path handles stereo signals (got %d)" % nc)
            data = np.asarray(aud.data, dtype=np.float64)
            L = data.shape[0]
            if self.sig_repr_params['transf'] != 'stft':
                # MinQT / CQT of both channels in one batched chain on the GPU
                # (audioModel.py:266-280), written straight into the engine's
                # resident observation: no F x T array reaches the host.
                # self.tft is left as after computeTransform(), without a host
                # copy of the last channel's transform
                F, T = self.tft.prepare_resident(L)
                self._engine = Engine(F, T, self.device)
                self._engine.set_audio_cqt(self.tft._context(), data)
                self.nbFreqsSigRepr, self.nbFramesSigRepr = F, T
                self._Cx = None
                self._finish_noise_limits()
                return
            hop = self.tft.fthop
            T = int(np.ceil(L / np.double(hop))) + 2
            F = self.tft.freqbins
            self._engine = Engine(F, T, self.device)
            self._engine.set_audio(data, self.tft.window, self.tft.ftlen, hop)
            self.tft.datalen_init = L
            self.nbFreqsSigRepr, self.nbFramesSigRepr = F, T
            self._Cx = None
        self._finish_noise_limits()

    def _finish_noise_limits(self):
        """Annealing limits from the mean diagonal PSD (audioModel.py:304-325)."""
        lim = self.noise['ann_PSD_lim']
        if lim[0] is None or lim[1] is None:
            mix_psd = self._engine.mix_psd()
            if lim[0] is None:
                lim[0] = np.real(mix_psd) / 100.
            if lim[1] is None:
                lim[1] = np.real(mix_psd) / 10000.
        if self.noise['sim_ann_opt'] in ('ann'):   # substring test, as the reference (:324)
            self.noise['PSD'] = lim[0]

    # ---------------------------------------------------------------- structure
    def _structure(self):
        """Check the model is on the HIP path; return (order, ranks, Ks, conv),
        order[j] = the keys of spatial component j's spectral components in
        the reference's key order (update_spectral_components iterates
        spec_comps.items(), audioModel.py:1479).

        HIP path: stereo; single-factor NMF spectral components (TW_constr
        'NMF'; FB, FW, TW each free or fixed; time blobs TB, free or fixed, or
        none), one or several per spatial component (comp_spat_comp_power sums
        them, :469-498); 'inst' and 'conv' spatial components in any
        combination the reference's mixing update can run (free 'conv' ones
        only when every component is free 'conv'); any lambdaCorr >= 0 (the
        inter-source correlation penalty, :1484-1719).

        Discrete-state time weights (TW_constr 'GSMM' / 'SHMM', :1728-1928):
        on a spectral component that is the only one of its spatial component
        (a constrained component sharing its spatial component with others
        raises NotImplementedError), with lambdaCorr == 0 (NotImplementedError
        otherwise) and no time blobs (AttributeError, as the reference :1736-
        1742), at most 4096 frequency bins (NotImplementedError from the
        upload: the device step keeps a frame tile of hat_W in LDS, DESIGN.md
        7.1).  The other spatial components of the model may carry any
        structure above.  'GMM' and 'HMM' raise NotImplementedError here,
        before any parameter moves: the reference updates the model and then
        raises from its first renormalisation (:2015,2038-2040).
        """
        if self.audioObject.channels != 2:
            raise AttributeError("Nb channels " + str(self.audioObject.channels) +
                                 " not implemented yet")
        J = len(self.spat_comps)
        if sorted(self.spat_comps.keys()) != list(range(J)):
            raise NotImplementedError("spatial components must be numbered 0..J-1")
        if self._is_sf():
            return self._structure_sf()
        owner = {}
        for k in sorted(self.spec_comps.keys()):
            comp = self.spec_comps[k]
            owner.setdefault(comp['spat_comp_ind'], []).append(k)
            facs = comp['factor']
            if list(facs.keys()) != [0]:
                raise NotImplementedError("spectral component %d: factor keys %s (a single factor "
                                          "has key 0)" % (k, list(facs.keys())))
            fac = facs[0]
            if len(fac['TB']):
                TB = np.asarray(fac['TB'])
                if TB.ndim != 2 or TB.shape[1] != self.nbFramesSigRepr or \
                        np.shape(fac['TW']) != (fac['FB'].shape[1], TB.shape[0]):
                    raise ValueError("time blobs of spectral component %d: TW %s, TB %s"
                                     % (k, np.shape(fac['TW']), TB.shape))
            constr = fac.get('TW_constr', 'NMF')
            if constr in ('GMM', 'HMM'):
                raise NotImplementedError(
                    "TW_constr=%s: Temporal discrete state mngmt not done yet. (the reference "
                    "raises this from renormalize_parameters, audioModel.py:2038-2040, after "
                    "its first update; refused here before any parameter moves)" % constr)
            if constr not in ('NMF', 'GSMM', 'SHMM'):
                raise NotImplementedError("TW_constr=%s is outside the HIP path" % constr)
            if constr != 'NMF' and fac.get('TW_frdm_prior', 'free') == 'free':
                if len(fac['TB']):
                    raise AttributeError(
                        "In this implementation, as in Ozerov's, non-trivial time blobs TB is "
                        "incompatible with discrete state-based constraints for the time "
                        "weights TW")
                if self.lambdaCorr > 0:
                    raise NotImplementedError("TW_constr=%s with lambdaCorr > 0 is outside the "
                                              "HIP path" % constr)
        if sorted(owner.keys()) != list(range(J)):
            raise NotImplementedError("every spatial component needs a spectral component")
        for j, keys in owner.items():
            if len(keys) > 1 and any(self._tw_constr(self.spec_comps[k]['factor'][0])
                                     for k in keys):
                raise NotImplementedError(
                    "a spectral component with discrete-state time weights must be the only one "
                    "of its spatial component on the HIP path (spatial component %d has %d)"
                    % (j, len(keys)))
        conv = [self.spat_comps[j]['mix_type'] == 'conv' for j in range(J)]
        free = [self.spat_comps[j]['frdm_prior'] == 'free' for j in range(J)]
        # update_mix_matrix (:843-863) solves the free 'conv' components with
        # the FULL hat_Rss[f] against the right-hand side of those components
        # only, which the reference can evaluate only when no other (fixed or
        # 'inst') component exists: any other component makes np.linalg.solve
        # raise at the first M-step.  Raise the same exception type up front.
        if any(c and f for c, f in zip(conv, free)) and not all(c and f for c, f in zip(conv, free)):
            raise ValueError("update_mix_matrix: free 'conv' spatial components next to fixed or "
                             "'inst' ones (audioModel.py:856-857 solves hat_Rss[f].T of all %d "
                             "components against the free components' right-hand side only)"
                             % J)
        ranks, Ks = [], []
        for j in range(J):
            p = self.spat_comps[j]['params']
            ranks.append(p.shape[0] if conv[j] else p.shape[1])
            Ks.append(int(sum(self.spec_comps[k]['factor'][0]['FB'].shape[1] for k in owner[j])))
        return [owner[j] for j in range(J)], ranks, Ks, (all(conv) if len(set(conv)) == 1 else conv)

    # ---------------------------------------------------------------- two factors
    SF_MAX_K = 128    # Kb, Kw of a factor on the two-factor path
    SF_MAX_RANK = 16  # total spatial rank: the explicit-V E-step k_suff_stat

    def _is_sf(self):
        """A model with a multi-factor spectral component: the two-factor
        (source / filter) path, fasst_sf.hip."""
        return any(len(c['factor']) > 1 for c in self.spec_comps.values())

    def _structure_sf(self):
        """The two-factor path: every spatial component has
        exactly one spectral component of one or two factors (keys 0 or 0, 1),
        each TW_constr 'NMF' without time blobs, FB F x Kb, FW Kb x Kw (not
        square in general), TW Kw x T with 1 <= Kb, Kw <= 128, FB / FW / TW
        independently free or fixed; lambdaCorr == 0; total spatial rank <=
        16; the spatial components as on the single-factor path.  Anything
        else raises NotImplementedError here, before any upload.  Returns
        (order, ranks, None, conv)."""
        J = len(self.spat_comps)
        what = "next to a two-factor spectral component"
        if self.lambdaCorr > 0:
            raise NotImplementedError("lambdaCorr > 0 %s is outside the HIP path" % what)
        owner = {}
        for k in sorted(self.spec_comps.keys()):
            comp = self.spec_comps[k]
            owner.setdefault(comp['spat_comp_ind'], []).append(k)
            keys = list(comp['factor'].keys())
            if len(keys) >= 3:
                raise NotImplementedError("spectral component %d has %d factors: the HIP path "
                                          "takes one or two" % (k, len(keys)))
            if keys not in ([0], [0, 1]):
                raise NotImplementedError("spectral component %d: factor keys %s (0 or 0, 1)"
                                          % (k, keys))
            for fi, fac in comp['factor'].items():
                if len(fac['TB']):
                    raise NotImplementedError("time blobs TB (spectral component %d factor %d) "
                                              "%s are outside the HIP path" % (k, fi, what))
                if fac.get('TW_constr', 'NMF') != 'NMF':
                    raise NotImplementedError("TW_constr=%s (spectral component %d factor %d): "
                                              "a discrete-state constraint %s is outside the HIP "
                                              "path" % (fac.get('TW_constr'), k, fi, what))
                shp = [np.shape(fac[p]) for p in ('FB', 'FW', 'TW')]
                if any(len(x) != 2 for x in shp) or shp[0][0] != self.nbFreqsSigRepr or \
                        shp[1][0] != shp[0][1] or shp[2][0] != shp[1][1] or \
                        shp[2][1] != self.nbFramesSigRepr:
                    raise ValueError("spectral component %d factor %d: FB %s, FW %s, TW %s for "
                                     "F=%d, T=%d" % ((k, fi) + tuple(shp) + (
                                         self.nbFreqsSigRepr, self.nbFramesSigRepr)))
                if min(shp[1]) >= 1 and shp[1][0] > self.SF_MAX_K and \
                        getattr(self, 'wideDictionary', False):
                    self._admit_wide(k, fi, fac, shp[1])
                elif min(shp[1]) < 1 or max(shp[1]) > self.SF_MAX_K:
                    raise NotImplementedError("spectral component %d factor %d: Kb=%d, Kw=%d "
                                              "outside 1..%d %s" % ((k, fi) + shp[1] + (
                                                  self.SF_MAX_K, what)))
        if sorted(owner.keys()) != list(range(J)):
            raise NotImplementedError("every spatial component needs a spectral component")
        for j, keys in owner.items():
            if len(keys) > 1:
                raise NotImplementedError("spatial component %d has %d spectral components: %s "
                                          "every spatial component takes exactly one"
                                          % (j, len(keys), what))
        conv = [self.spat_comps[j]['mix_type'] == 'conv' for j in range(J)]
        free = [self.spat_comps[j]['frdm_prior'] == 'free' for j in range(J)]
        if any(c and f for c, f in zip(conv, free)) and not all(c and f for c, f in zip(conv, free)):
            raise ValueError("update_mix_matrix: free 'conv' spatial components next to fixed or "
                             "'inst' ones (audioModel.py:856-857 solves hat_Rss[f].T of all %d "
                             "components against the free components' right-hand side only)" % J)
        ranks = []
        for j in range(J):
            p = self.spat_comps[j]['params']
            ranks.append(p.shape[0] if conv[j] else p.shape[1])
        # the device walks the components in spatial-component order, the
        # reference in key order: they differ only when a matrix is shared
        # (rescaled and updated in place, in order) and the map is not monotone
        own = [self.spec_comps[k]['spat_comp_ind'] for k in sorted(self.spec_comps.keys())]
        ids = [id(f[p]) for c in self.spec_comps.values() for f in c['factor'].values()
               for p in ('FB', 'FW', 'TW') if isinstance(f[p], np.ndarray)]
        if own != sorted(own) and len(ids) != len(set(ids)):
            raise NotImplementedError("a matrix shared between factors, with spectral component "
                                      "keys not in the order of their spatial components, %s is "
                                      "outside the HIP path" % what)
        if sum(ranks) > self.SF_MAX_RANK:
            raise NotImplementedError("total spatial rank %d above %d (the explicit-V E-step) %s"
                                      % (sum(ranks), self.SF_MAX_RANK, what))
        return [owner[j] for j in range(J)], ranks, None, conv

    SF_WIDE_MAX_K = 2048   # Kb of a wide factor (wideDictionary=True)

    def _admit_wide(self, k, fi, fac, shape):
        """The wide arm of the two-factor path ("Wide fixed
        dictionaries"): with self.wideDictionary set, a factor with 128 < Kb <=
        2048 whose FB and FW are fixed, FW square and diagonal, TW free.  FW
        is the identity where multiChanSourceF0Filter creates it; the
        renormalisation (the constructor's included) leaves a diagonal matrix
        in its place (FW *= max(FB), FW /= mean(FW), :2010-2018), so diagonal
        is what is compared here, on the host.  Anything else raises
        NotImplementedError, naming the factor and the property."""
        Kb, Kw = shape
        where = "spectral component %d factor %d (Kb=%d, Kw=%d)" % (k, fi, Kb, Kw)

        def refuse(prop):
            raise NotImplementedError("%s: %s; a wide dictionary (Kb > %d) is a fixed FB with a "
                                      "fixed, square, diagonal FW and a free NMF TW, Kb <= %d"
                                      % (where, prop, self.SF_MAX_K, self.SF_WIDE_MAX_K))
        if Kb > self.SF_WIDE_MAX_K:
            refuse("Kb above %d" % self.SF_WIDE_MAX_K)
        if fac.get('FB_frdm_prior', 'free') != 'fixed':
            refuse("FB_frdm_prior=%r" % fac.get('FB_frdm_prior', 'free'))
        if fac.get('FW_frdm_prior', 'fixed') != 'fixed':
            refuse("FW_frdm_prior=%r" % fac.get('FW_frdm_prior'))
        if Kw != Kb:
            refuse("FW is not square")
        FW = np.asarray(fac['FW'])
        if not np.all(np.isfinite(FW)) or np.count_nonzero(FW - np.diag(np.diag(FW))):
            refuse("FW is not diagonal")
        if fac.get('TW_frdm_prior', 'free') != 'free':
            refuse("TW_frdm_prior=%r" % fac.get('TW_frdm_prior'))

    def _refuse_sf(self, name):
        if self._is_sf():
            raise NotImplementedError("%s: not available on a model with a two-factor spectral "
                                      "component (DESIGN.md 7.2)" % name)

    def _upload_sf(self, order, ranks, conv):
        eng = self._engine
        factors, alias, seen = [], [], {}
        for j, keys in enumerate(order):
            facs = self.spec_comps[keys[0]]['factor']
            fl, al = [], []
            for i in sorted(facs.keys()):
                f = facs[i]
                fl.append((f['FB'].shape[1], np.shape(f['FW'])[1],
                           f.get('FB_frdm_prior', 'free') == 'free',
                           f.get('FW_frdm_prior', 'fixed') == 'free',
                           f.get('TW_frdm_prior', 'free') == 'free'))
                # one array object in several factors: one device buffer
                a = []
                for q, part in enumerate(('FB', 'FW', 'TW')):
                    key = (q, id(f[part]))
                    a.append(seen.get(key, -1) if isinstance(f[part], np.ndarray) else -1)
                    seen.setdefault(key, 2 * j + i)
                al.append(tuple(a))
            factors.append(fl)
            alias.append(al)
        key = (tuple(ranks), tuple(conv), repr(factors), repr(alias))
        if not eng.sf or getattr(eng, '_sf_key', None) != key:
            eng.sf_configure(ranks, conv, factors, alias)
            eng._sf_key = key
        for j, keys in enumerate(order):
            sc = self.spat_comps[j]
            eng.sf_set_spatial(j, sc['params'], sc['frdm_prior'] == 'free')
            facs = self.spec_comps[keys[0]]['factor']
            for i in sorted(facs.keys()):
                eng.set_factors(j, i, facs[i]['FB'], facs[i]['FW'], facs[i]['TW'])
        return order, None, conv

    def _download_sf(self, order, updated_spatial=True):
        eng = self._engine
        for j, keys in enumerate(order):
            sc = self.spat_comps[j]
            p = eng.sf_get_spatial(j, sc['params'].shape)
            if not np.iscomplexobj(sc['params']) and not (updated_spatial and
                                                          sc['frdm_prior'] == 'free'):
                p = p.real.copy()
            sc['params'] = p
            facs = self.spec_comps[keys[0]]['factor']
            for i in sorted(facs.keys()):
                for part, val in zip(('FB', 'FW', 'TW'), eng.get_factors(j, i)):
                    cur = facs[i][part]
                    if isinstance(cur, np.ndarray) and cur.shape == val.shape \
                            and cur.dtype == val.dtype and cur.flags.writeable:
                        cur[...] = val
                    else:
                        facs[i][part] = val

    def _renorm_factor_host(self, k, i, fac, ge, divide):
        """One factor's renormalisation on the host (audioModel.py:2006-2036,
        no time blobs), on its F x Kb, Kb x Kw and Kw x T matrices: used
        where the device cannot finish one (after a TW redraw) and for the
        initial state of multiChanSourceF0Filter.  Returns mean(TW), the
        `global_energy` the reference hands to the next factor."""
        fac['FB'] *= ge
        w = fac['FB'].max(axis=0)
        w[w == 0] = 1.
        fac['FB'] /= w
        fac['FW'] *= np.vstack(w)
        w = fac['FW'].mean(axis=0)
        w[w == 0] = 1.
        fac['FW'] /= w
        fac['TW'] *= np.vstack(w)
        if np.sum(fac['TW']) < eps:
            self._redraw_tw(k, i, fac)
        ge = fac['TW'].mean()
        if divide:
            fac['TW'] /= ge
        return ge

    def _redraw_tw(self, k, i, fac):
        fac['TW'] = np.random.randn(*fac['TW'].shape) ** 2
        fac['TW'] *= 1e3 * eps
        if self.verbose:
            print("    renorm: reinitialized TW for spec", k, "factor", i)

    def _restart_tw_sf(self, mask, order):
        """The random TW restart (audioModel.py:2023-2028) and the rest of the
        component's renormalisation (:2034-2036), in key-then-factor order;
        bit 2 j + i of mask is factor i of spatial component j.  The reference
        hands mean(TW) of a factor to the next one as its energy, so the
        device leaves the factors after a dead one alone: they are
        renormalised here, with the mean of the redrawn TW."""
        spat = {order[j][0]: j for j in range(len(order))}
        for k in sorted(self.spec_comps.keys()):
            facs = self.spec_comps[k]['factor']
            keys = sorted(facs.keys())
            for n, i in enumerate(keys):
                if not mask & (1 << (2 * spat[k] + i)):
                    continue
                self._redraw_tw(k, i, facs[i])
                ge = facs[i]['TW'].mean()
                if i < len(facs) - 1:
                    facs[i]['TW'] /= ge
                for i2 in keys[n + 1:]:
                    ge = self._renorm_factor_host(k, i2, facs[i2], ge, i2 < len(facs) - 1)
                break

    @staticmethod
    def _tw_constr(fac):
        """'GSMM' / 'SHMM' when the factor's TW step is the discrete-state one
        (free TW, audioModel.py:1634,1728), else None."""
        c = fac.get('TW_constr', 'NMF')
        return c if c in ('GSMM', 'SHMM') and fac.get('TW_frdm_prior', 'free') == 'free' else None

    def _constrained(self, order):
        """[(spatial component, spectral key, factor, constraint)] of the
        discrete-state components."""
        out = []
        for j, keys in enumerate(order):
            fac = self.spec_comps[keys[0]]['factor'][0]
            if len(keys) == 1 and self._tw_constr(fac):
                out.append((j, keys[0], fac, self._tw_constr(fac)))
        return out

    def _upload(self):
        order, ranks, Ks, conv = self._structure()
        if Ks is None:
            return self._upload_sf(order, ranks, conv)
        eng = self._engine
        eng.configure(ranks, Ks, conv)
        for j in range(len(order)):
            sc = self.spat_comps[j]
            eng.set_spatial(j, sc['params'], sc['frdm_prior'] == 'free')
            facs = [self.spec_comps[k]['factor'][0] for k in order[j]]
            fb_free = [f.get('FB_frdm_prior', 'free') == 'free' for f in facs]
            fw_free = [f.get('FW_frdm_prior', 'fixed') == 'free' for f in facs]
            tw_free = [f.get('TW_frdm_prior', 'free') == 'free' for f in facs]
            # a component with time blobs: the device forms H = TW.TB (fasst_set_tb)
            TWs = [np.zeros((f['FB'].shape[1], self.nbFramesSigRepr)) if len(f['TB'])
                   else f['TW'] for f in facs]
            if len(facs) == 1:
                FB, FW, TW = facs[0]['FB'], facs[0]['FW'], TWs[0]
            else:   # the components side by side, FW block diagonal
                FB = np.hstack([f['FB'] for f in facs])
                TW = np.vstack(TWs)
                FW = np.zeros((Ks[j], Ks[j]))
                a = 0
                for f in facs:
                    n = f['FB'].shape[1]
                    FW[a:a + n, a:a + n] = f['FW']
                    a += n
            eng.set_spectral(j, FB, FW, TW, any(fb_free), any(tw_free), any(fw_free))
            eng.set_blocks(j, np.cumsum([0] + [f['FB'].shape[1] for f in facs]), fb_free, fw_free,
                           tw_free)
            for b, f in enumerate(facs):
                if len(f['TB']):
                    eng.set_tb(j, b, f['TW'], f['TB'], f.get('TB_frdm_prior') == 'free')
            constr = self._tw_constr(facs[0]) if len(facs) == 1 else None
            # TW_all / TW_DP_params when the factor already has them, else the
            # reference's first-use values formed by the library (:1744-1760)
            eng.set_tw_constr(j, constr or 'NMF', facs[0].get('TW_all'),
                              facs[0].get('TW_DP_params'),
                              facs[0].get('TW_DP_frdm_prior') == 'free')
        if self.lambdaCorr > 0:   # components one at a time in key order (:1479)
            pos = {k: (j, b) for j, keys in enumerate(order) for b, k in enumerate(keys)}
            seq = [pos[k] for k in sorted(self.spec_comps.keys())]
            eng.set_corr(self.lambdaCorr, [j for j, _ in seq], [b for _, b in seq])
        else:
            eng.set_corr(0.0)
        return order, Ks, conv

    def _download_constr(self, order, iters=1):
        """After TW steps: TW_all / TW_DP_params into the factor dicts as the
        reference leaves them (:1744-1760,1809,1902-1924), the last decoded
        state sequences into self.tw_state_seq[spectral key], and the
        reference's unconditional print per prior update (:1903)."""
        for j, k, fac, constr in self._constrained(order):
            TW_all, dp, state = self._engine.get_tw_constr(j, constr)
            fac['TW_all'] = TW_all
            fac['TW_DP_params'] = dp
            if not hasattr(self, 'tw_state_seq'):
                self.tw_state_seq = {}
            self.tw_state_seq[k] = state
            if fac.get('TW_DP_frdm_prior') == 'free':
                for _ in range(iters):
                    print("    Updating the transition probabilities")

    def _warn_constr(self, order):
        if self._constrained(order):   # the reference's warning (:1729-1731)
            warnings.warn("The GMM/GSMM/HMM still needs to be adapted " +
                          "to take into account the different factors. ")

    def _download(self, order, Ks, conv, updated_spatial=True):
        if Ks is None:
            return self._download_sf(order, updated_spatial)
        eng = self._engine
        for j in range(len(order)):
            sc = self.spat_comps[j]
            p = eng.get_spatial(j, sc['params'].shape)
            if not np.iscomplexobj(sc['params']) and not (updated_spatial and
                                                          sc['frdm_prior'] == 'free'):
                p = p.real.copy()
            sc['params'] = p
            FB, FW, TW = eng.get_spectral(j, Ks[j])
            a = 0
            for b, k in enumerate(order[j]):
                fac = self.spec_comps[k]['factor'][0]
                n = fac['FB'].shape[1]
                parts = (('FB', FB[:, a:a + n]), ('FW', FW[a:a + n, a:a + n]),
                         ('TW', TW[a:a + n]))
                if len(fac['TB']):   # the factor TW and TB, not H
                    TWs, TB = eng.get_tb(j, b, n, np.shape(fac['TB'])[0])
                    parts = parts[:2] + (('TW', TWs), ('TB', TB))
                if len(order[j]) > 1:
                    parts = tuple((key, np.ascontiguousarray(val)) for key, val in parts)
                for key, val in parts:
                    if isinstance(fac[key], np.ndarray) and fac[key].shape == val.shape \
                            and fac[key].dtype == val.dtype:
                        fac[key][...] = val
                    else:
                        fac[key] = val
                a += n

    def _restart_tw(self, mask, order):
        """Random TW restart of renormalize_parameters (audioModel.py:2023-2028),
        drawn on the host RNG in spectral-component key order; mask has one bit
        per spectral component, spatial component by spatial component."""
        if self._is_sf():
            return self._restart_tw_sf(mask, order)
        dead = set()
        bit = 0
        for keys in order:
            for k in keys:
                if mask & (1 << bit):
                    dead.add(k)
                bit += 1
        for k in sorted(self.spec_comps.keys()):
            if k in dead:
                fac = self.spec_comps[k]['factor'][0]
                fac['TW'] = np.random.randn(*fac['TW'].shape) ** 2
                fac['TW'] *= 1e3 * eps
                if self.verbose:
                    print("    renorm: reinitialized TW for spec", k, "factor", 0)
                if len(fac['TB']):   # the rest of the renormalisation (:2029-2033)
                    w = fac['TB'].mean(axis=1)
                    w[w == 0] = 1.
                    fac['TB'] /= np.vstack(w)
                    fac['TW'] *= w

    # ---------------------------------------------------------------- EM
    def _annealed_psd(self, i):
        lim = self.noise['ann_PSD_lim']
        return ((np.sqrt(lim[0]) * (self.iter_num - i) + np.sqrt(lim[1]) * i)
                / self.iter_num) ** 2

    def estim_param_a_post_model(self,):
        """Run iter_num GEM iterations on the GPU (audioModel.py:330-382)."""
        logliks = np.ones(self.iter_num)
        opt = self.noise['sim_ann_opt']
        if opt in ['ann', ]:
            self.noise['PSD'] = self.noise['ann_PSD_lim'][0]
        elif opt == 'no_ann':
            self.noise['PSD'] = self.noise['ann_PSD_lim'][1]
        else:
            warnings.warn("To add noise to the signal, provide the " +
                          "sim_ann_opt from any of 'ann', " + "'no_ann' or 'ann_ns_inj' ")
        rows = []
        for i in range(self.iter_num):
            if opt in ['ann', 'ann_ns_inj']:
                rows.append(self._annealed_psd(i))
            else:
                rows.append(np.asarray(self.noise['PSD'], dtype=np.float64) *
                            np.ones(self.nbFreqsSigRepr))
        if not rows:
            return logliks
        rows = np.array(rows, dtype=np.float64)
        order, Ks, conv = self._upload()
        self._warn_constr(order)
        i0 = 0
        while i0 < self.iter_num:
            ll, done, mask = self._engine.run(rows[i0:], self.nmfUpdateCoeff)
            logliks[i0:i0 + done] = ll
            i0 += done
            self._download_constr(order, done)
            if mask:
                self._download(order, Ks, conv)
                self._restart_tw(mask, order)
                order, Ks, conv = self._upload()
        self._download(order, Ks, conv)
        self.noise['PSD'] = rows[-1]
        if self.verbose:
            for i in range(self.iter_num):
                print("Iteration", i + 1, "on", self.iter_num, "    log-likelihood:", logliks[i])
        return logliks

    def GEM_iteration(self,):
        """One GEM iteration with the current noise PSD (audioModel.py:384-428)."""
        order, Ks, conv = self._upload()
        psd = np.asarray(self.noise['PSD'], dtype=np.float64) * np.ones(self.nbFreqsSigRepr)
        self._warn_constr(order)
        ll, done, mask = self._engine.run(psd[None, :], self.nmfUpdateCoeff)
        self._download(order, Ks, conv)
        self._download_constr(order, done)
        if mask:
            self._restart_tw(mask, order)
        return ll[0]

    def renormalize_parameters(self):
        """renormalize_parameters on the GPU (audioModel.py:1980-2040)."""
        order, Ks, conv = self._upload()
        mask = self._engine.renormalize()
        self._download(order, Ks, conv, updated_spatial=False)
        if mask:
            self._restart_tw(mask, order)

    # ---------------------------------------------------------------- GEM steps
    # The methods GEM_iteration is made of (audioModel.py:384-428), each a
    # device call on the reference's own arrays (fasst_steps.hip).  GEM_iteration
    # itself runs the fused iteration (fasst_run) and never materialises them.
    def _psd_row(self):
        return np.asarray(self.noise['PSD'], dtype=np.float64) * np.ones(self.nbFreqsSigRepr)

    def retrieve_subsrc_params(self,):
        """(spat_comp_powers [R, F, T], mix_matrix [R, 2, F], rank_part_ind)
        (audioModel.py:514-578); the powers come from the device."""
        self._refuse_sf('retrieve_subsrc_params')
        order, Ks, conv = self._upload()
        J = len(order)
        rank_part_ind, total = {}, 0
        for j in range(J):
            sc = self.spat_comps[j]
            rank = sc['params'].shape[1] if sc['mix_type'] == 'inst' else sc['params'].shape[0]
            rank_part_ind[j] = total + np.arange(rank)
            total += rank
        V = self._engine.source_powers(0, J)
        spat_comp_powers = np.empty((total, self.nbFreqsSigRepr, self.nbFramesSigRepr))
        mix_matrix = np.zeros((total, self.audioObject.channels, self.nbFreqsSigRepr),
                              dtype=complex)
        for j in range(J):
            sc = self.spat_comps[j]
            spat_comp_powers[rank_part_ind[j]] = V[j]
            if sc['mix_type'] == 'inst':
                mix_matrix[rank_part_ind[j]] = np.asarray(sc['params']).T[:, :, None]
            else:
                mix_matrix[rank_part_ind[j]] = sc['params']
        return spat_comp_powers, mix_matrix, rank_part_ind

    def compute_suff_stat(self, spat_comp_powers, mix_matrix):
        """(hat_Rxx, hat_Rxs, hat_Rss, hat_Ws, loglik) on the device
        (audioModel.py:580-764), with the current noise PSD."""
        if self.audioObject.channels != 2:
            raise ValueError("Nb channels not supported:" + str(self.audioObject.channels))
        if self._engine is None:
            raise AttributeError("no observation: call comp_transf_Cx() first")
        return self._engine.suff_stat(spat_comp_powers, mix_matrix, self._psd_row())

    def update_mix_matrix(self, hat_Rxs, hat_Rss, mix_matrix, rank_part_ind):
        """Mixing update (audioModel.py:766-889): mix_matrix updated in place,
        the free spatial components' params replaced."""
        kind = np.zeros(mix_matrix.shape[0], dtype=np.int32)
        for j, sc in self.spat_comps.items():
            if sc['frdm_prior'] == 'free':
                kind[rank_part_ind[j]] = 1 if sc['mix_type'] == 'inst' else 2
        m = np.ascontiguousarray(mix_matrix, dtype=np.complex128)
        self._engine.mix_solve(hat_Rss, hat_Rxs, m, kind)
        if m is not mix_matrix:
            mix_matrix[...] = m
        for j, sc in self.spat_comps.items():
            if sc['frdm_prior'] == 'free':
                if sc['mix_type'] == 'inst':
                    sc['params'] = np.mean(mix_matrix[rank_part_ind[j]], axis=2).T
                else:
                    sc['params'] = mix_matrix[rank_part_ind[j]]

    def update_spectral_components(self, hat_W):
        """FB / FW / TW (TB) updates from hat_W [J, F, T] on the device
        (audioModel.py:1469-1978); no renormalisation.  NotImplementedError on
        a model with a two-factor spectral component, as retrieve_subsrc_params,
        compute_sigma_comp_2d and comp_spat_cmps_powers: the piecewise steps
        exist for the single-factor path only (estim_param_a_post_model,
        GEM_iteration, renormalize_parameters and the separation run)."""
        self._refuse_sf('update_spectral_components')
        order, Ks, conv = self._upload()
        self._warn_constr(order)
        self._engine.spectral_update(hat_W, self.nmfUpdateCoeff)
        self._download(order, Ks, conv, updated_spatial=False)
        self._download_constr(order)

    def _colmask(self, spat_ind, spec_comp_ind, order):
        keys = spec_comp_ind if len(spec_comp_ind) else order[spat_ind]
        mask, a = 0, 0
        for k in order[spat_ind]:
            n = self.spec_comps[k]['factor'][0]['FB'].shape[1]
            if k in keys:
                mask |= ((1 << n) - 1) << a
            a += n
        return mask

    def compute_sigma_comp_2d(self, spat_ind, spec_comp_ind):
        """(sigma_comp_diag [2, F, T], sigma_comp_off [F, T]) of one spatial
        component's spectral components (audioModel.py:1327-1372)."""
        self._refuse_sf('compute_sigma_comp_2d')
        order, Ks, conv = self._upload()
        return self._engine.sigma_comp(spat_ind, self._colmask(spat_ind, spec_comp_ind, order))

    def compute_inv_sigma_mix_2d(self, sigma_comps_diag, sigma_comps_off):
        """Inverse of sum_n Sigma_n + PSD I (audioModel.py:1374-1394)."""
        return self._engine.inv_sigma_mix(sigma_comps_diag, sigma_comps_off, self._psd_row())

    def compute_Wiener_gain_2d(self, sigma_comp_diag, sigma_comp_off, inv_sigma_mix_diag,
                               inv_sigma_mix_off, timeInvariant=False):
        """WG [2, 2, F(, T)] (audioModel.py:1396-1467)."""
        from .engine import wiener_gain
        dev = self._engine.device if self._engine is not None else \
            (0 if self.device is None else self.device)
        return wiener_gain(dev, sigma_comp_diag, sigma_comp_off, inv_sigma_mix_diag,
                           inv_sigma_mix_off)

    # ---------------------------------------------------------------- NMF init
    def _mono_power(self):
        """Channel-averaged power sum_c Re Cx[c, c] / nc (audioModel.py:2150-2158)."""
        nc = self.audioObject.channels
        Cx = np.copy(np.real(self.Cx[0]))
        Cx += np.real(self.Cx[2])
        Cx /= np.double(nc)
        return Cx

    def initialize_all_spec_comps_with_NMF(self, sameInitAll=False, **kwargs):
        """IS-NMF of the mono power initialises FB / TW (audioModel.py:2091-2116);
        the NMF iterations and the renormalisation run on the GPU."""
        if sameInitAll:
            return self.initialize_all_spec_comps_with_NMF_same(**kwargs)
        return self.initialize_all_spec_comps_with_NMF_indiv(**kwargs)

    def initialize_all_spec_comps_with_NMF_indiv(self, niter=10, updateFreqBasis=True,
                                                 updateTimeWeight=True, **kwargs):
        """One NMF over all components, started from the current FB / TW
        (audioModel.py:2118-2177)."""
        from .tools.nmf import NMF_decomp_init
        nbSpecComps = [sc['factor'][0]['FB'].shape[1] for sc in self.spec_comps.values()]
        total = int(np.sum(nbSpecComps))
        FBinit = np.zeros([self.nbFreqsSigRepr, total])
        TWinit = np.zeros([total, self.nbFramesSigRepr])
        for k, sc in self.spec_comps.items():
            a = int(np.sum(nbSpecComps[:k]))
            FBinit[:, a:a + nbSpecComps[k]] = sc['factor'][0]['FB']
            TWinit[a:a + nbSpecComps[k]] = sc['factor'][0]['TW']
        W, H = NMF_decomp_init(SX=self._mono_power(), nbComps=total, niter=niter,
                               verbose=self.verbose, Winit=FBinit, Hinit=TWinit,
                               updateW=updateFreqBasis, updateH=updateTimeWeight,
                               device=self.device)
        for k, sc in self.spec_comps.items():
            a = int(np.sum(nbSpecComps[:k]))
            if updateFreqBasis:
                sc['factor'][0]['FB'] = np.maximum(W[:, a:a + nbSpecComps[k]], eps)
            if updateTimeWeight:
                sc['factor'][0]['TW'] = np.maximum(H[a:a + nbSpecComps[k]], eps)
        self.renormalize_parameters()

    def initialize_all_spec_comps_with_NMF_same(self, niter=10, **kwargs):
        """One NMF, the same W / H (most energetic first) for every component
        (audioModel.py:2179-2222)."""
        from .tools.nmf import NMF_decomposition
        if not np.all([len(sc['factor']) == 1 for sc in self.spec_comps.values()]):
            raise NotImplementedError("NMF init not implemented for multi factor models.")
        nbSpecComps = [sc['factor'][0]['FB'].shape[1] for sc in self.spec_comps.values()]
        W, H = NMF_decomposition(SX=self._mono_power(), verbose=self.verbose,
                                 nbComps=int(np.max(nbSpecComps)), niter=niter,
                                 device=self.device)
        indexSort = np.argsort(H.sum(axis=1))[::-1]
        W = W[:, indexSort]
        H = H[indexSort]
        for sc in self.spec_comps.values():
            n = sc['factor'][0]['FB'].shape[1]
            sc['factor'][0]['FB'][:] = W[:, :n]
            sc['factor'][0]['TW'][:] = H[:n]
        self.renormalize_parameters()

    # ---------------------------------------------------------------- separation
    def separate_spat_comps(self, dir_results=None, suffix=None):
        """One source per spatial component (audioModel.py:1063-1086)."""
        spec_comp_ind = {}
        for spat_ind in range(len(self.spat_comps)):
            spec_comp_ind[spat_ind] = []
        for spec_ind, spec_comp in self.spec_comps.items():
            spec_comp_ind[spec_comp['spat_comp_ind']].append(spec_ind)
        self.separate_comps(dir_results=dir_results, spec_comp_ind=spec_comp_ind, suffix=suffix)

    def separated_images(self, spec_comp_ind=None):
        """STFT-domain Wiener images S[n, c] = sum_c2 WG_n[c, c2] X[c2], as the
        reference computes before its iSTFT (audioModel.py:1136-1214)."""
        if self._is_sf():
            src_of, psd = self._separation_plan_sf(spec_comp_ind)
            return self._engine.sf_wiener_images(psd, src_of)
        src_spat, psd = self._separation_plan(spec_comp_ind)
        S = self._engine.wiener_images(psd)
        return S[src_spat]

    def separated_waveforms(self, spec_comp_ind=None):
        """The per-source, per-channel inverse transform of separated_images()
        without the images leaving the GPU: [n, channel, sample], trimmed to
        the input length as tft.invertTransform() does (audioModel.py:1187-1217,
        tftransforms/stft.py:71-131).  With a MinQT / CQT every image goes
        through one batched inverse chain (minqt.py:794-868, :1013-1055)."""
        t = self.tft
        if getattr(t, 'transformname', None) != 'stft':
            cqt, L = self._resident_cqt()
            if self._is_sf():
                src_of, psd = self._separation_plan_sf(spec_comp_ind)
                return self._engine.sf_separate_waveforms_cqt(cqt, psd, src_of, L)
            src_spat, psd = self._separation_plan(spec_comp_ind)
            return self._engine.separate_waveforms_cqt(cqt, psd, L)[src_spat]
        if self._is_sf():
            src_of, psd = self._separation_plan_sf(spec_comp_ind)
            Y = self._engine.sf_separate_waveforms(psd, src_of, t.synthWindow, t.window, t.ftlen,
                                                   t.fthop)
            return Y[:, :, :t.datalen_init]
        src_spat, psd = self._separation_plan(spec_comp_ind)
        Y = self._engine.separate_waveforms(psd, t.synthWindow, t.window, t.ftlen, t.fthop)
        return Y[src_spat][:, :, :t.datalen_init]

    def _resident_cqt(self):
        """(device context, signal length) of the rasterised MinQT / CQT whose
        frame bookkeeping tft holds (comp_transf_Cx or computeTransform)."""
        t = self.tft
        t._check_attr_inversion()
        return t._context(), int(t.datalen_init)

    def _separation_plan_sf(self, spec_comp_ind):
        """Two-factor model: upload, and (src_of, last annealed PSD), src_of[j]
        = the source that spatial component j's spectral component belongs to
        (-1: none).  The per-bin Wiener filter runs from the V_j planes with
        the formulas of compute_sigma_comp_2d / compute_inv_sigma_mix_2d /
        compute_Wiener_gain_2d (audioModel.py:1327-1467)."""
        if spec_comp_ind is None:
            spec_comp_ind = {n: [n] for n in range(len(self.spec_comps))}
        order, Ks, conv = self._upload()
        spat = {keys[0]: j for j, keys in enumerate(order)}
        src_of = [-1] * len(order)
        for n in range(len(spec_comp_ind)):
            for k in spec_comp_ind[n]:
                if src_of[spat[k]] not in (-1, n):
                    raise NotImplementedError("a spectral component in two separation sources "
                                              "is outside the two-factor path")
                src_of[spat[k]] = n
        if max(src_of) != len(spec_comp_ind) - 1:
            raise ValueError("separation sources must each hold a spectral component")
        psd = np.asarray(self.noise['PSD'], dtype=np.float64) * np.ones(self.nbFreqsSigRepr)
        return src_of, psd

    def _separation_plan(self, spec_comp_ind):
        """Set the engine's separation sources; return (output order, last
        annealed PSD).  Source n holds the spectral components spec_comp_ind[n]
        (default: one source per spectral component, audioModel.py:1130-1133):
        Sigma_n sums, per spatial component, R_j times the power of those of
        its components (compute_sigma_comp_2d, :1327-1372) and Sigma_x sums
        the sources (compute_inv_sigma_mix_2d, :1374-1394).  Sources that are
        whole spatial components, all of them, take the per-spatial-component
        kernel (outputs reordered); others the source-table kernel."""
        if spec_comp_ind is None:
            spec_comp_ind = {}
            for spec_ind in range(len(self.spec_comps)):
                spec_comp_ind[spec_ind] = [spec_ind, ]
        order, Ks, conv = self._upload()
        col = {}
        for j, keys in enumerate(order):
            a = 0
            for k in keys:
                n = self.spec_comps[k]['factor'][0]['FB'].shape[1]
                col[k] = (j, a, n)
                a += n
        sources = []
        for n in range(len(spec_comp_ind)):
            terms = {}
            for k in spec_comp_ind[n]:
                j, a, w = col[k]
                terms[j] = terms.get(j, 0) | (((1 << w) - 1) << a)
            sources.append(sorted(terms.items()))
        full = [(j, (1 << Ks[j]) - 1) for j in range(len(order))]
        whole = all(len(t) == 1 and t[0] == full[t[0][0]] for t in sources)
        psd = np.asarray(self.noise['PSD'], dtype=np.float64) * np.ones(self.nbFreqsSigRepr)
        if whole and sorted(t[0][0] for t in sources) == list(range(len(order))):
            self._engine.set_sources(None)
            return [t[0][0] for t in sources], psd
        self._engine.set_sources(sources)
        return list(range(len(sources))), psd

    def separate_comps(self, dir_results=None, spec_comp_ind=None, suffix=None):
        """Wiener-filter and write one WAV per source (audioModel.py:1088-1236)."""
        if dir_results is None:
            dir_results = '/'.join(self.audioObject.filename.split('/')[:-1])
        nc = self.audioObject.channels
        if nc != 2:
            raise NotImplementedError()
        Y = self.separated_waveforms(spec_comp_ind)   # inverse transform on the device
        nbSources = Y.shape[0]
        if not hasattr(self, "files"):
            self.files = {}
        self.files['spat_comp'] = []
        fileroot = self.audioObject.filename.split('/')[-1][:-4]
        for n in range(nbSources):
            ndata = Y[n].T
            _suffix = ''
            if suffix is not None and n in suffix:
                _suffix = '_' + suffix[n]
            outAudioName = (dir_results + '/' + fileroot + '_' + str(n) + '-' +
                            str(nbSources) + _suffix + '.wav')
            self.files['spat_comp'].append(outAudioName)
            out = ao.AudioObject(filename=outAudioName, mode='w')
            out._data = np.int16(ndata[:self.audioObject.nframes, :] * self.audioObject._maxdata)
            out._maxdata = 1
            out._encoding = 'pcm16'
            out.samplerate = self.audioObject.samplerate
            out._write()

    # ---------------------------------------------------------------- spatial filter
    def _spatial_filter_plan(self):
        """The reference's refusals (audioModel.py:947-949, :965-966), then the
        parameters on the device."""
        self._refuse_sf('separate_spatial_filter_comp')
        if self.audioObject.channels != 2:
            raise NotImplementedError()
        for n in range(len(self.spat_comps)):
            if self.spat_comps[n]['mix_type'] == 'inst':
                raise NotImplementedError('Mixing params not convolutive...')
        self._upload()

    def spatial_filter_gains(self):
        """Time-invariant gains WG[n] = R_n inv(mean_n R_n) / Re trace, [J, 2, 2, F],
        of the 'conv' mixing parameters (audioModel.py:959-1004)."""
        self._spatial_filter_plan()
        return self._engine.spatial_filter_gains()

    def spatial_filter_images(self):
        """Images S[n, c] = sum_c2 WG[n][c, c2] X[c2], [J, 2, F, T], as the
        reference forms them before each inverse transform (audioModel.py:1015-1030)."""
        self._spatial_filter_plan()
        return self._engine.spatial_filter_images()

    def spatial_filter_waveforms(self):
        """The inverse transform of spatial_filter_images() with the gains
        applied as the device inverse loads the observation (the iSTFT's frame
        loader; the MinQT / CQT inverse's raster gather, all 2 J images in one
        batched chain): [J, channel, sample], trimmed as tft.invertTransform()
        does."""
        t = self.tft
        self._spatial_filter_plan()
        if getattr(t, 'transformname', None) != 'stft':
            cqt, L = self._resident_cqt()
            return self._engine.spatial_filter_waveforms_cqt(cqt, L)
        Y = self._engine.spatial_filter_waveforms(t.synthWindow, t.window, t.ftlen, t.fthop)
        return Y[:, :, :t.datalen_init]

    def separate_spatial_filter_comp(self, dir_results=None, suffix=None):
        """Separate with the spatial filter of the mixing parameters alone, one
        WAV per spatial component (audioModel.py:891-1061).  With the STFT the
        gains are applied inside the device iSTFT, with a MinQT / CQT inside
        the batched device inverse."""
        if dir_results is None:
            dir_results = '/'.join(self.audioObject.filename.split('/')[:-1])
        self._spatial_filter_plan()
        Y = self.spatial_filter_waveforms()
        nbSources = Y.shape[0]
        if not hasattr(self, 'files'):
            self.files = {}
        self.files['spatial'] = []
        fileroot = self.audioObject.filename.split('/')[-1][:-4]
        for n in range(nbSources):
            ndata = Y[n].T
            _suffix = '_spatial'
            if suffix is not None and n in suffix:
                _suffix += '_' + suffix[n]
            outAudioName = (dir_results + '/' + fileroot + '_' + str(n) + '-' +
                            str(nbSources) + _suffix + '.wav')
            self.files['spatial'].append(outAudioName)
            out = ao.AudioObject(filename=outAudioName, mode='w')
            out._data = np.int16(ndata[:self.audioObject.nframes, :] * self.audioObject._maxdata)
            out._maxdata = 1
            out._encoding = 'pcm16'
            out.samplerate = self.audioObject.samplerate
            out._write()

    def gcc_phat_tdoa_2d(self):
        """GCC-PHAT detection function irfft(Cx[1] / |Cx[1]|, n=fsize, axis=0)
        (audioModel.py:1316-1324): on the device for the STFT, the reference's
        NumPy expression on Cx for the other transforms (their bins are no
        half-spectrum of fsize)."""
        if self.sig_repr_params['transf'] == 'stft' and self._engine is not None:
            return self._engine.gcc_phat(self.sig_repr_params['fsize'])
        with np.errstate(invalid='ignore', divide='ignore'):   # 0/0 = NaN, as the reference
            return np.fft.irfft(self.Cx[1] / np.abs(self.Cx[1]),
                                n=self.sig_repr_params['fsize'], axis=0)

    def dir_diag_stereo(self, ntheta=512, distanceInterMic=0.3):
        """Capon directivity diagram of the model's own observation: what
        spatial.steering_vectors.dir_diag_stereo(self.Cx, nft=fsize,
        samplerate=...) returns, from the resident planes (no F x T array
        crosses to the host).  Not a method of the reference's class."""
        if self._engine is None:
            raise AttributeError("no observation: call comp_transf_Cx() first")
        return self._engine.dir_diag(ntheta, distanceInterMic, self.sig_repr_params['fsize'],
                                     self._samplerate_or_default())

    def mvdr_2d(self, theta, distanceInterMic=.3):
        """The reference's method (audioModel.py:1238-1314) cannot run, so there
        is nothing to reproduce: its steering-vector module uses `np` and
        `soundCelerity` without defining either (spatial/steering_vectors.py:48-52)
        and it ends in `ao.filter_stft`, which audioObject does not have.
        Kept for the class surface."""
        raise NotImplementedError(
            "mvdr_2d: the reference's method cannot run (spatial/steering_vectors.py:48-52 "
            "has neither numpy nor soundCelerity in scope, and audioObject.filter_stft does "
            "not exist), so no result exists to reproduce; use separate_spatial_filter_comp()")

    # ---------------------------------------------------------------- helpers
    def comp_spat_comp_power(self, spat_comp_ind, spec_comp_ind=[], factor_ind=[]):
        """Host-side V = prod_factors (FB.FW).(TW[.TB]) (audioModel.py:430-498);
        a parameter inspection helper, not used by the GPU iteration."""
        V = np.zeros([self.nbFreqsSigRepr, self.nbFramesSigRepr])
        keys = spec_comp_ind if len(spec_comp_ind) else list(self.spec_comps.keys())
        for k in keys:
            if spat_comp_ind != self.spec_comps[k]['spat_comp_ind']:
                continue
            Vc = np.ones([self.nbFreqsSigRepr, self.nbFramesSigRepr])
            facs = factor_ind if len(factor_ind) else list(self.spec_comps[k]['factor'].keys())
            for fi in facs:
                fac = self.spec_comps[k]['factor'][fi]
                H = np.dot(fac['TW'], fac['TB']) if len(fac['TB']) else fac['TW']
                Vc *= np.dot(np.dot(fac['FB'], fac['FW']), H)
            V += Vc
        return V

    def comp_spat_cmps_powers(self, spat_comp_ind, spec_comp_ind=[], factor_ind=[]):
        """Sum of the spectral powers of the spatial components listed in
        spat_comp_ind (audioModel.py:500-512; spec_comp_ind / factor_ind are
        accepted and unused, as there).  Each component's power comes from
        the device (fasst_source_powers on the uploaded parameters) and the
        sum runs on the host in the list's order."""
        self._refuse_sf('comp_spat_cmps_powers')
        self._upload()
        V = 0
        for i in spat_comp_ind:
            V += self._engine.source_powers(int(i), 1)[0]
        return V

    def setComponentParameter(self, newValue, spec_ind, fact_ind=0, partLabel='FB',
                              prior='free', keepDimensions=True):
        """The reference's unfinished helper (audioModel.py:2042-2089): it
        prints its notice, then its first statement reads the misspelt name
        `keepDimenstions` and raises NameError before touching anything.
        Kept as that behaviour so the class surface is the same; set the
        components directly (spec_comps[k]['factor'][f][...]), as its notice
        says."""
        print("NOT IMPLEMENTED YET, PLEASE SET THE COMPONENTS DIRECTLY")
        raise NameError("name 'keepDimenstions' is not defined")

    def initializeConvParams(self, initMethod='demix'):
        """Convolutive spatial parameters (audioModel.py:2224-2294): every
        spatial component becomes 'conv'; 'rand' draws the steering vectors
        A = randn(J, F, nc) + 1j randn(J, F, nc) from the global np.random
        stream (the reference's draw order) and gives every rank of
        component j the parameters A[j].T.  'demix' needs the DEMIX
        estimator (pyfasst.demixTF), which is outside this engine's scope
        (DESIGN.md §7): NotImplementedError.  The method is checked before
        any component changes type (the reference sets every 'mix_type' to
        'conv' first, so a caught error left 'conv' components holding 'inst'
        parameters): a refused call leaves the model as it was."""
        nc = self.audioObject.channels
        for spat_ind, spat_comp in self.spat_comps.items():
            if spat_comp['mix_type'] != 'inst':
                warnings.warn("Spatial component %d " % spat_ind +
                              "already not instantaneous, overwriting...")
        if initMethod == 'demix':
            raise NotImplementedError("initializeConvParams('demix'): the DEMIX estimator "
                                      "(demixTF) is outside the HIP engine's scope; use 'rand'")
        elif 'rand' not in initMethod:
            raise ValueError("Init method not implemented.")
        J = len(self.spat_comps)
        A = (np.random.randn(J, self.nbFreqsSigRepr, nc) +
             1j * np.random.randn(J, self.nbFreqsSigRepr, nc))
        for spat_comp in self.spat_comps.values():
            spat_comp['mix_type'] = 'conv'
        for nspat, (spat_ind, spat_comp) in enumerate(self.spat_comps.items()):
            spat_comp['params'] = np.zeros([self.rank[nspat], nc, self.nbFreqsSigRepr],
                                           dtype=complex)
            for r in range(self.rank[nspat]):
                spat_comp['params'][r] = A[spat_ind].T


class MultiChanNMFInst_FASST(FASST):
    """Multichannel NMF, instantaneous mixing (audioModel.py:2296-2420)."""

    def __init__(self, audio, nbComps=3, nbNMFComps=4, spatial_rank=2, **kwargs):
        super(MultiChanNMFInst_FASST, self).__init__(audio=audio, **kwargs)
        self.comp_transf_Cx()
        self.nbComps = nbComps
        self.nbNMFComps = nbNMFComps
        self.rank = np.atleast_1d(spatial_rank)
        if self.rank.size < self.nbComps:
            self.rank = [self.rank[0], ] * self.nbComps
        self._initialize_structures()

    def _initialize_structures(self):
        """Initial parameters; consumes the global np.random stream in the
        reference's order (audioModel.py:2349-2393)."""
        nc = self.audioObject.channels
        self.spat_comps = {}
        self.spec_comps = {}
        for j in range(self.nbComps):
            self.spat_comps[j] = {}
            self.spat_comps[j]['time_dep'] = 'indep'
            self.spat_comps[j]['mix_type'] = 'inst'
            self.spat_comps[j]['frdm_prior'] = 'free'
            self.spat_comps[j]['params'] = np.random.randn(nc, self.rank[j])
            if nc == 2:
                self.spat_comps[j]['params'] = (
                    np.array([np.sin((j + 1) * np.pi / (2. * (self.nbComps + 1))) +
                              np.random.randn(self.rank[j]) * np.sqrt(0.01),
                              np.cos((j + 1) * np.pi / (2. * (self.nbComps + 1))) +
                              np.random.randn(self.rank[j]) * np.sqrt(0.01)]))
            self.spec_comps[j] = {}
            self.spec_comps[j]['spat_comp_ind'] = j
            self.spec_comps[j]['factor'] = {}
            fac = {}
            fac['FB'] = 0.75 * np.abs(np.random.randn(self.nbFreqsSigRepr, self.nbNMFComps)) + 0.25
            fac['FW'] = np.eye(self.nbNMFComps)
            fac['TW'] = 0.75 * np.abs(np.random.randn(self.nbNMFComps, self.nbFramesSigRepr)) + 0.25
            fac['TB'] = []
            fac['FB_frdm_prior'] = 'free'
            fac['FW_frdm_prior'] = 'fixed'
            fac['TW_frdm_prior'] = 'free'
            fac['TB_frdm_prior'] = []
            fac['TW_constr'] = 'NMF'
            self.spec_comps[j]['factor'][0] = fac
        self.renormalize_parameters()

    def setSpecCompFB(self, compNb, FB, FB_frdm_prior='fixed'):
        """audioModel.py:2395-2420"""
        speccomp = self.spec_comps[compNb]['factor'][0]
        if self.nbFreqsSigRepr != FB.shape[0]:
            raise AttributeError("Size of provided FB is not consistent" + " with inner attributes")
        speccomp['FB'] = np.copy(FB)
        ncomp = FB.shape[1]
        speccomp['FW'] = np.eye(ncomp)
        speccomp['TW'] = 0.75 * np.abs(np.random.randn(ncomp, self.nbFramesSigRepr)) + 0.25
        speccomp['FB_frdm_prior'] = FB_frdm_prior


class MultiChanNMFConv(MultiChanNMFInst_FASST):
    """Convolutive multichannel NMF (audioModel.py:2422-2508)."""

    def __init__(self, audio, nbComps=3, nbNMFComps=4, spatial_rank=2, **kwargs):
        super(MultiChanNMFConv, self).__init__(audio=audio, nbComps=nbComps,
                                               nbNMFComps=nbNMFComps,
                                               spatial_rank=spatial_rank, **kwargs)

    def makeItConvolutive(self):
        """Replicate the instantaneous params over bins (audioModel.py:2488-2508)."""
        nc = self.audioObject.channels
        for nspat, (spat_ind, spat_comp) in enumerate(self.spat_comps.items()):
            if spat_comp['mix_type'] != 'inst':
                warnings.warn("Spatial component %d " % spat_ind +
                              "already not instantaneous, skipping...")
            else:
                spat_comp['mix_type'] = 'conv'
                inst = spat_comp['params']
                p = np.zeros([self.rank[nspat], nc, self.nbFreqsSigRepr], dtype=complex)
                p[:] = inst.T[:, :, None]
                spat_comp['params'] = p


class MultiChanHMM(MultiChanNMFConv):
    """A MultiChanNMFConv whose time weights can be turned into hidden Markov
    model state sequences (audioModel.py:2510-2549)."""

    def __init__(self, audio, nbComps=3, nbNMFComps=4, spatial_rank=2, **kwargs):
        super(MultiChanHMM, self).__init__(audio=audio, nbComps=nbComps,
                                           nbNMFComps=nbNMFComps,
                                           spatial_rank=spatial_rank, **kwargs)

    def makeItHMM(self):
        """HMM time constraints (audioModel.py:2525-2532).  The reference's
        'HMM' cannot complete an iteration (renormalize_parameters raises,
        :2038-2040); estimation refuses it up front."""
        for spec_ind, spec_comp in self.spec_comps.items():
            for fac_ind, factor in spec_comp['factor'].items():
                factor['TW_constr'] = 'HMM'
                factor['TW_DP_frdm_prior'] = 'free'

    def makeItSHMM(self):
        """SHMM time constraints (audioModel.py:2534-2549): transitions
        9 I + 1, row-normalised, fixed."""
        for spec_ind, spec_comp in self.spec_comps.items():
            for fac_ind, factor in spec_comp['factor'].items():
                nbfaccomps = factor['TW'].shape[0]
                factor['TW_constr'] = 'SHMM'
                factor['TW_DP_params'] = 9 * np.eye(nbfaccomps)
                factor['TW_DP_params'] += 1.
                factor['TW_DP_params'] /= np.vstack(factor['TW_DP_params'].sum(axis=1))
                factor['TW_DP_frdm_prior'] = 'fixed'


class multiChanSourceF0Filter(FASST):
    """Multichannel source / filter model (audioModel.py:2551-3014): nbComps - 1
    components whose power is a source factor (the F0 comb dictionary, TW free)
    times a filter factor (Hann bumps, FW nbFilterComps x nbFilterWeigs and TW
    free), and one residual NMF component.  Runs on the two-factor path
    (fasst_sf.hip); the dictionaries are built on the GPU.

    On the device every factor has Kb, Kw <= 128 (FASST._structure_sf) unless
    the model is created with wideDictionary=True.  The reference's default
    F0 range and step (minF0=39, maxF0=2000, stepnoteF0=16) give a source
    dictionary of 1093 columns: the model can be constructed (its initial
    renormalisation runs on the host), but by default (wideDictionary=False)
    estim_param_a_post_model() and the separation still refuse it by name.
    wideDictionary=True admits the source factor at up to 2048 columns (fixed
    FB, fixed diagonal FW, free TW: FASST._admit_wide) and runs it on the wide
    arm of fasst_sf.hip; the sparsity reweighting takes such a
    model as it is.  With `sparsity` set (the median filter length of each
    component's F0 track) the reference's schedule runs on the device as its
    own loop body, GEM_iteration() then reweigh_sparsity_constraint(sigma)
    (k_sf_bary / k_sf_sparsify), or resident through Engine.sf_run_sparse;
    the fused estim_param_a_post_model() raises NotImplementedError for such
    a model and names both.  initializeFreeMats() starts the source
    activations from an IS-NMF of the mono power on the source dictionary, at
    any dictionary width.  initSpecCompsWithLabelAndFiles and the
    multichanLead subclass are outside the scope."""

    def __init__(self, audio, nbComps=3, nbNMFResComps=1, nbFilterComps=20, nbFilterWeigs=[4, ],
                 minF0=39, maxF0=2000, minF0search=80, maxF0search=800, stepnoteF0=16,
                 chirpPerF0=1, spatial_rank=1, sparsity=None, wideDictionary=False, **kwargs):
        from .SeparateLeadStereo import separateLeadFunctions as slf
        super(multiChanSourceF0Filter, self).__init__(audio=audio, **kwargs)
        self.wideDictionary = bool(wideDictionary)
        self.comp_transf_Cx()
        self.sourceParams = {'minF0': minF0, 'maxF0': maxF0, 'stepnoteF0': stepnoteF0,
                             'chirpPerF0': chirpPerF0, 'minF0search': minF0search,
                             'maxF0search': maxF0search, }
        self.nbComps = nbComps
        self.nbNMFResComps = nbNMFResComps
        self.nbFilterComps = nbFilterComps
        if len(nbFilterWeigs) < self.nbComps - 1:
            self.nbFilterWeigs = [nbFilterWeigs[0], ] * self.nbComps
        else:
            self.nbFilterWeigs = nbFilterWeigs
        self.spatial_rank = np.atleast_1d(spatial_rank)
        if self.spatial_rank.size < self.nbComps:
            self.spatial_rank = [self.spatial_rank[0], ] * self.nbComps
        # the source dictionary, shared by every component (:2616-2637)
        self.F0Table, WF0, trfoBis = slf.generate_WF0_TR_chirped(
            transform=self.tft, minF0=minF0, maxF0=maxF0, stepNotes=stepnoteF0, Ot=0.5,
            perF0=chirpPerF0, depthChirpInSemiTone=0.5, loadWF0=True, verbose=self.verbose,
            device=self.device)
        WF0 = np.array(WF0, dtype=np.float64)
        for nwf0comp in range(WF0.shape[1]):   # low-energy bins to eps (:2627-2629)
            indLowEnergy = np.where(WF0[:, nwf0comp] < WF0[:, nwf0comp].max() * 1e-4)
            WF0[indLowEnergy, nwf0comp] = eps
        self.sourceFreqComps = np.ascontiguousarray(
            np.hstack([WF0[:self.nbFreqsSigRepr], np.vstack(np.ones(self.nbFreqsSigRepr))]))
        del WF0
        self.nbSourceComps = self.sourceFreqComps.shape[1]
        self.sourceFreqWeights = np.eye(self.nbSourceComps)
        self.filterFreqComps = slf.generateHannBasis(
            numberFrequencyBins=self.nbFreqsSigRepr, sizeOfFourier=self.sig_repr_params['fsize'],
            Fs=self.audioObject.samplerate, frequencyScale='linear',
            numberOfBasis=self.nbFilterComps)
        self.sparsity = sparsity
        self._initialize_structures()

    def _initialize_structures(self, seed=None):
        """Initial parameters, the reference's draw order on the global
        np.random stream (audioModel.py:2650-2772).  The source dictionary and
        its weights are ONE array in every source / filter component, as in
        the reference, whose renormalisation rescales them in place component
        after component: the device keeps one buffer for them too."""
        np.random.seed(seed)
        self.rank = self.spatial_rank
        nc = self.audioObject.channels
        sparsity = self.sparsity
        self.spat_comps = {}
        self.spec_comps = {}
        F, T = self.nbFreqsSigRepr, self.nbFramesSigRepr

        def factor(FB, FW, TW, fb, fw):
            return {'FB': FB, 'FW': FW, 'TW': TW, 'TB': [], 'FB_frdm_prior': fb,
                    'FW_frdm_prior': fw, 'TW_frdm_prior': 'free', 'TB_frdm_prior': [],
                    'TW_constr': 'NMF'}
        for j in range(self.nbComps - 1):
            self.spat_comps[j] = {'time_dep': 'indep', 'mix_type': 'inst', 'frdm_prior': 'free'}
            self.spat_comps[j]['params'] = np.random.randn(nc, self.rank[j])
            if nc == 2:
                self.spat_comps[j]['params'] = (
                    np.array([np.sin((j + 1) * np.pi / (2. * (self.nbComps))) +
                              np.random.randn(self.rank[j]) * np.sqrt(0.01),
                              np.cos((j + 1) * np.pi / (2. * (self.nbComps))) +
                              np.random.randn(self.rank[j]) * np.sqrt(0.01)]))
            self.spec_comps[j] = {'spat_comp_ind': j, 'factor': {}}
            TW0 = 0.75 * np.abs(np.random.randn(self.nbSourceComps, T)) + 0.25
            self.spec_comps[j]['factor'][0] = factor(self.sourceFreqComps, self.sourceFreqWeights,
                                                     TW0, 'fixed', 'fixed')
            FW1 = 0.75 * np.abs(np.random.randn(self.nbFilterComps, self.nbFilterWeigs[j])) + 0.25
            TW1 = 0.75 * np.abs(np.random.randn(self.nbFilterWeigs[j], T)) + 0.25
            self.spec_comps[j]['factor'][1] = factor(self.filterFreqComps, FW1, TW1, 'fixed',
                                                     'free')
        self.resSpatialRank = self.rank[-1]
        j = self.nbComps - 1
        self.spat_comps[j] = {'time_dep': 'indep', 'mix_type': 'inst', 'frdm_prior': 'free'}
        self.spat_comps[j]['params'] = np.random.randn(nc, self.resSpatialRank)
        self.spec_comps[j] = {'spat_comp_ind': j, 'factor': {}}
        FB = 0.75 * np.abs(np.random.randn(F, self.nbNMFResComps)) + 0.25
        TW = 0.75 * np.abs(np.random.randn(self.nbNMFResComps, T)) + 0.25
        self.spec_comps[j]['factor'][0] = factor(FB, np.eye(self.nbNMFResComps), TW, 'free',
                                                 'fixed')
        if sparsity is None or len(sparsity) not in (1, self.nbComps):
            for j in range(self.nbComps):
                self.spec_comps[j]['sparsity'] = False
        elif len(sparsity) == self.nbComps:
            for j in range(self.nbComps):
                self.spec_comps[j]['sparsity'] = sparsity[j]
        else:
            for j in range(self.nbComps):
                self.spec_comps[j]['sparsity'] = sparsity[0]
        self._renormalize_host()

    def _renormalize_host(self):
        """renormalize_parameters (audioModel.py:1980-2040) of the initial
        state, on the host: a few F x Kb, Kb x Kw and Kw x T matrices, once.
        It keeps the constructor usable for any dictionary size (the device
        path takes Kb, Kw <= 128 and says so when the estimation starts) and
        applies the reference's in-place rescaling of the shared source
        dictionary as written."""
        energy = {}
        for j, sc in self.spat_comps.items():
            energy[j] = np.mean(np.abs(sc['params']) ** 2)
            sc['params'] /= np.sqrt(energy[j])
        for k, comp in self.spec_comps.items():
            ge = energy[comp['spat_comp_ind']]
            nfac = len(comp['factor'])
            for i, fac in comp['factor'].items():
                ge = self._renorm_factor_host(k, i, fac, ge, i < nfac - 1)

    def setSpecCompFB(self, compNb, FB, FB_frdm_prior='fixed', ):
        """audioModel.py:2858-2876"""
        speccomp = self.spec_comps[compNb]['factor'][0]
        if self.nbFreqsSigRepr != FB.shape[0]:
            raise AttributeError("Size of provided FB is not consistent" + " with inner attributes")
        speccomp['FB'] = np.copy(FB)
        ncomp = FB.shape[1]
        speccomp['FW'] = np.eye(ncomp)
        speccomp['TW'] = 0.75 * np.abs(np.random.randn(ncomp, self.nbFramesSigRepr)) + 0.25
        speccomp['FB_frdm_prior'] = FB_frdm_prior

    def initializeFreeMats(self, niter=10):
        """audioModel.py:2878-2908: IS-NMF of the mono power on the fixed
        source dictionary (NMF_decomp_init with updateW=False, on the GPU at
        any dictionary width), the activations shared out in place over the
        source / filter components, then the renormalisation (on the host, as
        the constructor's).  The residual component is left as it is."""
        from .tools.nmf import NMF_decomp_init
        W, H = NMF_decomp_init(SX=self._mono_power(),
                               Winit=np.dot(self.sourceFreqComps,
                                            self.spec_comps[0]['factor'][0]['FW']),
                               verbose=self.verbose, nbComps=self.nbSourceComps, niter=niter,
                               updateW=False, updateH=True, device=self.device)
        for ncomp in range(self.nbComps - 1):
            self.spec_comps[ncomp]['factor'][0]['TW'][:] = np.copy(H) / (self.nbComps - 1)
        self._renormalize_host()

    def makeItConvolutive(self):
        """audioModel.py:2910-2931"""
        nc = self.audioObject.channels
        for nspat, (spat_ind, spat_comp) in enumerate(self.spat_comps.items()):
            if spat_comp['mix_type'] != 'inst':
                warnings.warn("Spatial component %d " % spat_ind +
                              "already not instantaneous, skipping...")
            else:
                spat_comp['mix_type'] = 'conv'
                inst = spat_comp['params']
                p = np.zeros([self.rank[nspat], nc, self.nbFreqsSigRepr], dtype=complex)
                p[:] = np.atleast_2d(inst.T)[:, :, None]
                spat_comp['params'] = p

    def estim_param_a_post_model(self, ):
        """audioModel.py:2933-2979 for sparsity=None (reweigh_sparsity_constraint
        then does nothing): the base class's iterations on the GPU, fused in
        one device call.  With a sparsity constraint the fused call is refused
        (NotImplementedError): the schedule runs as the reference's own loop
        body (:2966-2977),

            for i in range(iter_num):
                logliks[i] = model.GEM_iteration()
                model.reweigh_sparsity_constraint(sigma_i)

        with sigma_i = exp(log K^2 + (log 9 - log K^2) i / max(iter_num - 1, 1)),
        K the largest factor-0 TW.shape[0] of the spectral components, both
        steps on the device; Engine.sf_run_sparse runs the whole schedule
        without the parameters leaving the GPU."""
        if any(sc.get('sparsity') for sc in self.spec_comps.values()):
            raise NotImplementedError(
                "multiChanSourceF0Filter with a sparsity constraint: the fused "
                "estim_param_a_post_model() does not run the sparsity schedule "
                "(audioModel.py:2939-2977); loop over GEM_iteration() and "
                "reweigh_sparsity_constraint(sigma), or use Engine.sf_run_sparse")
        return super(multiChanSourceF0Filter, self).estim_param_a_post_model()

    def reweigh_sparsity_constraint(self, sigma):
        """audioModel.py:2981-3014 on the device (fasst_sf_reweigh): for j in
        range(nbComps), where spec_comps[j]['sparsity'] is set and factor 0's
        TW has more than two rows, TW is multiplied in place by the Gaussian
        mask of width sigma centred on the barycentre of its columns over the
        F0 axis, median-filtered over spec_comps[j]['sparsity'] frames (the
        mask's last row, the unvoiced one, holds the column maximum; columns
        are divided by that maximum where it is > 0).  Uploads the model, runs
        k_sf_bary and k_sf_sparsify per component, and writes the reweighed TW
        back into the model's arrays; nothing happens when no component
        qualifies."""
        lengths = {}
        for j in range(self.nbComps):
            comp = self.spec_comps[j]
            L = comp['sparsity']
            if L and comp['factor'][0]['TW'].shape[0] > 2:
                if int(L) != L or L < 0:
                    raise ValueError("spec_comps[%d]['sparsity'] = %r is not a median filter "
                                     "length (an integer > 0)" % (j, L))
                lengths[comp['spat_comp_ind']] = (j, int(min(L, 2 ** 31 - 1)))
        if not lengths:
            return
        if self.audioObject.channels != 2:
            raise AttributeError("Nb channels " + str(self.audioObject.channels) +
                                 " not implemented yet")
        order, ranks, _, conv = self._structure_sf()
        self._upload_sf(order, ranks, conv)
        eng = self._engine
        eng.sf_set_sparsity([lengths.get(j, (0, 0))[1] for j in range(len(order))])
        eng.sf_reweigh(sigma)
        for j, (k, _) in sorted(lengths.items()):
            self.spec_comps[k]['factor'][0]['TW'][...] = eng.get_factors(j, 0, tw_only=True)
