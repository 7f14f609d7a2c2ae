"""DEMIX on the GPU (demixTF.py of the reference): counts and locates the
sources of a stereo mixture from their spatial cues and returns, per source,
`theta` (the relative amplitude between the channels) and `delta` (their
relative delay in samples) [Arberet2010]_.

    Arberet, S.; Gribonval, R. & Bimbot, F.
    A Robust Method to Count and Locate Audio Sources in
    a Multichannel Underdetermined Mixture
    IEEE Transactions on Signal Processing, 2010, 58, 121 - 133

Signatures, attribute names and quirks are the reference's (DESIGN.md §7.9
lists the quirks).  The feature planes `confidence`, `thetaAll`, `phiAll`,
`thetaVarAll`, the set `subTFpointSet` of points still to classify and the
cluster masks `clusters` live on the device (include/fasst_demix.h,
pyfasst_amd/csrc/fasst_demix.hip): reading one of these attributes downloads a
copy, assigning to it uploads, and neither `comp_clusters()` nor
`refine_clusters()` moves a plane to the host -- a clustering round moves the
centroid's four numbers, three sums per bin and two counts.  Changing a
downloaded array in place does not change the device's; assign it back.

What raises NotImplementedError: a `tfrepresentation` other than 'stft' /
'stftold' (the reference's other branch of compute_temporal is its "slower,
may not work" kernel product), `refine_clusters()` with `nsources=None`
(remove_weak_clusters, TFPoint.clusterDistBound) and `spatial_filtering()`.
"""
import ctypes
import warnings

import numpy as np

from . import _lib
from . import audioObject as ao
from ._lib import check, dptr, iptr, lib
from .tftransforms import tft
from .tftransforms.stft import stft as _stft

eps = 1e-10

# global variables
uVarBound = 2.33
uDistBound = 2.33

_PLANES = {'confidence': 0, 'thetaAll': 1, 'phiAll': 2, 'thetaVarAll': 3}


def decibel(val):
    return 20. * np.log10(val)


# alias for above function:
db = decibel


def invdb(dbval):
    return 10. ** (dbval / 20.)


def get_indices_peak(sequence, ind_max, threshold=0.8):
    """returns the indices of the peak around ind_max,
    with values down to  ``threshold * sequence[ind_max]``
    (the sequence is circular)
    """
    thres_value = sequence[ind_max] * threshold
    lenSeq = sequence.size
    indSup = ind_max
    indInf = ind_max
    while sequence[indSup] > thres_value:
        indSup += 1
        indSup = np.remainder(indSup, lenSeq)
    while sequence[indInf] > thres_value:
        indInf -= 1
        indInf = np.remainder(indInf, lenSeq)
    indices = np.zeros(lenSeq, dtype=bool)
    if indInf < indSup:
        indices[(indInf + 1):indSup] = True
    else:
        indices[:indSup] = True
        indices[(indInf + 1):] = True
    return indices


def confidenceFromVar(variance, neighbors):
    """Computes the confidence, in dB, for a given number of
    neighbours and a variance.
    """
    with np.errstate(all='ignore'):
        alpha = ((2 * variance * (neighbors - 1) + 1 +
                  np.sqrt(1 + 4 * variance * (neighbors - 1)))
                 / (2 * variance * (neighbors - 1)))
        return 20 * np.log10(alpha)


def launch_count():
    """Kernels of fasst_demix.hip launched by this process so far."""
    n = ctypes.c_long(0)
    check(lib.demix_launch_count(ctypes.byref(n)), "demix_launch_count")
    return n.value


def transfer_count():
    """[F, L] planes and masks copied to the host by this process so far."""
    n = ctypes.c_long(0)
    check(lib.demix_transfer_count(ctypes.byref(n)), "demix_transfer_count")
    return n.value


def last_ms():
    """Device time (HIP events) of the kernels of the last device call."""
    ms = np.zeros(1)
    check(lib.demix_last_ms(dptr(ms)), "demix_last_ms")
    return float(ms[0])


def _plane_property(name):
    which = _PLANES[name]

    def get(self):
        ctx = self._need_ctx(name)
        out = np.empty((self._F, self._L))
        check(lib.demix_get_plane(ctx, which, dptr(out)), "demix_get_plane")
        return out

    def put(self, value):
        ctx = self._need_ctx(name)
        a = np.ascontiguousarray(value, dtype=np.float64)
        if a.shape != (self._F, self._L):
            raise ValueError("%s: shape %s, the planes are %s" % (name, a.shape,
                                                                  (self._F, self._L)))
        check(lib.demix_set_plane(ctx, which, dptr(a)), "demix_set_plane")

    return property(get, put)


class DEMIX(object):
    """DEMIX algorithm, for 2 channels."""

    def __init__(self, audio,
                 nsources=2,
                 wlen=2048,
                 hopsize=1024,
                 neighbors=20,
                 verbose=0,
                 maxclusters=100,
                 tfrepresentation='stft',
                 tffmin=25, tffmax=18000,
                 tfbpo=48,
                 winFunc=tft.sqrt_blackmanharris,
                 device=None):
        self.nsources = nsources
        if nsources is None:
            self.maxclusters = maxclusters
        else:
            self.maxclusters = np.maximum(maxclusters, self.nsources * 10)
        self.verbose = verbose
        self.neighbors = neighbors
        if isinstance(audio, ao.AudioObject):
            self.audioObject = audio
        elif isinstance(audio, str):
            self.audioObject = ao.AudioObject(filename=audio)
        else:
            raise AttributeError("The provided audio parameter is" +
                                 "not a supported format.")
        self.device = _lib.default_device() if device is None else device
        self.sig_repr_params = {}
        self.sig_repr_params['wlen'] = wlen
        self.sig_repr_params['fsize'] = ao.nextpow2(wlen)
        self.sig_repr_params['hopsize'] = hopsize
        self.sig_repr_params['tfrepresentation'] = tfrepresentation.lower()
        self.sig_repr_params['hopfactor'] = 1. * hopsize / self.sig_repr_params['wlen']
        self.sig_repr_params['tftkwargs'] = {
            'fmin': tffmin, 'fmax': tffmax, 'bins': tfbpo,
            'linFTLen': self.sig_repr_params['fsize'],
            'fs': self.audioObject.samplerate,
            'atomHopFactor': self.sig_repr_params['hopfactor'],
            'winFunc': winFunc
            }
        if self.sig_repr_params['tfrepresentation'] not in ('stft', 'stftold'):
            raise NotImplementedError(
                "DEMIX: tfrepresentation %r; the clustering runs on 'stft' and 'stftold' (the "
                "detection function of the other transforms is the reference's untested kernel "
                "product)" % (tfrepresentation,))
        self.tft = tft.tftransforms[self.sig_repr_params['tfrepresentation']](
            device=self.device, **self.sig_repr_params['tftkwargs'])
        self._ctx = None
        self._F = self._L = 0
        self._slots = []
        self._have_subset = False
        # device time of the last feature stage and of each clustering round (ms),
        # each round's cluster size and the points left after it (the device's counts)
        self.features_ms = 0.
        self.round_ms = []
        self.round_pass_ms = []  # (argmax, theta pass, delta pass) of each round
        self.round_sizes = []
        self.round_remaining = []

    # ---------------------------------------------------------------- device
    def _need_ctx(self, what):
        if self._ctx is None:
            raise AttributeError("DEMIX has no %s yet (comp_pcafeatures first)" % what)
        return self._ctx

    def _free_ctx(self):
        if getattr(self, '_ctx', None) is not None:
            lib.demix_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self._free_ctx()
        except Exception:
            pass

    confidence = _plane_property('confidence')
    thetaAll = _plane_property('thetaAll')
    phiAll = _plane_property('phiAll')
    thetaVarAll = _plane_property('thetaVarAll')

    def _get_mask(self, slot):
        out = np.empty((self._F, self._L), dtype=np.uint8)
        check(lib.demix_get_mask(self._ctx, slot, out.ctypes.data_as(_lib._ucp)), "demix_get_mask")
        return out.astype(bool)

    def _set_mask(self, slot, value):
        a = np.ascontiguousarray(np.asarray(value, dtype=bool), dtype=np.uint8)
        if a.shape != (self._F, self._L):
            raise ValueError("mask of shape %s, the planes are %s" % (a.shape, (self._F, self._L)))
        check(lib.demix_set_mask(self._ctx, slot, a.ctypes.data_as(_lib._ucp)), "demix_set_mask")

    def _get_subset(self):
        self._need_ctx('subTFpointSet')
        if not self._have_subset:
            raise AttributeError("DEMIX has no subTFpointSet yet (init_subpts_set first)")
        return self._get_mask(-1)

    def _set_subset(self, value):
        self._need_ctx('subTFpointSet')
        self._set_mask(-1, value)
        self._have_subset = True

    subTFpointSet = property(_get_subset, _set_subset)

    def _get_clusters(self):
        if '_slots_set' not in self.__dict__:
            raise AttributeError("'DEMIX' object has no attribute 'clusters'")
        return [self._get_mask(s) for s in self._slots]

    def _set_clusters(self, value):
        value = list(value)
        if len(value):
            self._need_ctx('clusters')
        if len(value) > self.maxclusters:
            raise ValueError("%d clusters, the device keeps %d" % (len(value), self.maxclusters))
        for n, m in enumerate(value):
            self._set_mask(n, m)
        self._slots = list(range(len(value)))
        self._sizes = [int(np.sum(m)) for m in value]
        self._slots_set = True

    clusters = property(_get_clusters, _set_clusters)

    # -------------------------------------------------------------- clustering
    def comp_clusters(self, threshold=0.8):
        """Computes the time-frequency clusters, along with their centroids,
        which contain the parameters of the mixing process - namely `theta`,
        which parameterizes the relative amplitude, and `delta`, which is
        homogeneous to a delay in samples between the two channels.
        """
        self.comp_sig_repr()
        self.comp_pcafeatures()
        self.comp_parameters()
        self.init_subpts_set()

        self.clusterCentroids = []
        self._slots = []
        self._sizes = []
        self._slots_set = True
        self.round_ms = []
        self.round_pass_ms = []
        self.round_sizes = []
        self.round_remaining = []
        nbRemainingPoints = self._F * self._L
        if self.verbose:
            print("Computing the clusters... ", nbRemainingPoints, "TF points")
        while nbRemainingPoints and len(self._slots) < self.maxclusters:
            centroid = self.get_max_confidence_point()
            ms_argmax = last_ms()
            self.clusterCentroids.append(centroid)
            sums, distBound = self._theta_pass(centroid)
            ms_theta = last_ms()
            maxDelta = self._identify_deltaT(sums, centroid, threshold)
            slot = len(self._slots)
            if maxDelta is not None:
                centroid.delta = maxDelta
                size, nbRemainingPoints = self._delta_pass(slot, centroid, only_centroid=False)
            else:
                centroid.delta = np.nan
                # keeping only the centroid in that cluster, then:
                size, nbRemainingPoints = self._delta_pass(slot, centroid, only_centroid=True)
            ms_delta = last_ms()
            ms = ms_argmax + ms_theta + ms_delta
            self.round_pass_ms.append((ms_argmax, ms_theta, ms_delta))
            self.round_ms.append(ms)
            self.round_sizes.append(size)
            self.round_remaining.append(nbRemainingPoints)
            self._slots.append(slot)
            self._sizes.append(size)
            if self.verbose > 1:
                print("comp_clusters:")
                print("    ***theta***:", centroid.theta)
                print("    ***delta***:", maxDelta)
                print("    cluster size", size, "remaining", nbRemainingPoints)

    def refine_clusters(self):
        """Refining the clusters in order to verify that they are possible.
        With self.nsources given, this method only keeps that number of
        clusters (the best ones)."""
        if self.nsources is None:
            raise NotImplementedError(
                "DEMIX.refine_clusters with nsources=None (remove_weak_clusters, "
                "TFPoint.clusterDistBound) is not implemented; give nsources")
        self.reestimate_clusterCentroids()
        self.keepBestClusters()
        self.reestimate_clusterCentroids()

    def _centroid_dist_bound(self, centroid_tfpoint):
        with np.errstate(all='ignore'):
            distBound = np.sqrt(
                self.estim_bound_var_theta(centroid_tfpoint.confidence,
                                           infOrSup='sup',
                                           u=uVarBound)
                ) * uDistBound
            # conversion to angle on the sphere (???)
            return 1 / 2. * np.arccos(((distBound ** 2 - 2) ** 2) / 2. - 1)

    def _theta_pass(self, centroid_tfpoint):
        distBound = self._centroid_dist_bound(centroid_tfpoint)
        sums = np.empty((self._F, 3))
        check(lib.demix_theta_pass(self._need_ctx('features'), float(centroid_tfpoint.theta),
                                   float(distBound), dptr(sums)), "demix_theta_pass")
        return sums, distBound

    def getTFpointsNearTheta_OneScale(self, centroid_tfpoint):
        """returns the TF points whose theta is close to that of the centroid,
        among the points still to classify, and the bound on the distance:
        the candidate mask of the device pass, downloaded."""
        _, distBound = self._theta_pass(centroid_tfpoint)
        if not self._have_subset:
            raise AttributeError("DEMIX has no subTFpointSet yet (init_subpts_set first)")
        return self._get_mask(-2), distBound

    def _host_sums(self, ind_cluster_pts):
        """The per-bin sums of compute_temporal for a mask given by the
        caller, on downloaded planes (the clustering loop takes them from the
        device pass)."""
        ind_cluster_pts = np.asarray(ind_cluster_pts, dtype=bool)
        with np.errstate(all='ignore'):
            thetaVars = self.thetaVarAll
            thetaVars[thetaVars == 0] = eps
            y = (1 / thetaVars) * np.exp(1j * self.phiAll)
            thetaVars[~ind_cluster_pts] = np.inf
            y[~ind_cluster_pts] = 0
            sums = np.empty((self._F, 3))
            ysum = y.sum(axis=1)
            sums[:, 0], sums[:, 1] = ysum.real, ysum.imag
            sums[:, 2] = np.sum((1 / thetaVars), axis=1)
        return sums

    def _detection_function(self, sums, zoom):
        """compute_temporal from the per-bin sums of the device pass."""
        with np.errstate(all='ignore'):
            normalisation = np.array(sums[:, 2])
            normalisation[normalisation == 0] = eps
            y = sums[:, 0] + 1j * sums[:, 1]
            return np.fft.irfft(y / normalisation, n=self.sig_repr_params['fsize'] * zoom)

    def compute_temporal(self, ind_cluster_pts, zoom):
        """This computes the inverse Fourier transform of the
        estimated Steering Vectors, weighed by their inverse variance.
        Host form on downloaded planes, for a mask given by the caller; the
        clustering loop takes the sums from the device pass."""
        return self._detection_function(self._host_sums(ind_cluster_pts), zoom)

    def _identify_deltaT(self, sums, centroid, threshold):
        with np.errstate(all='ignore'):
            distBound = centroid.estimDeltaPhi()
            # max nb of samples in error interval:
            nbMaxSamples = 2 ** 7
            # max zoom for oversampling
            zoomMax = 2 ** 4
            if distBound != np.inf:
                zoom = 2 ** np.ceil(np.log2(nbMaxSamples / 2 * distBound))
                zoom = max(1, zoom)
                zoom = min(zoom, zoomMax)
                zoom = int(zoom)
            else:
                zoom = 1
            ind_candidates = centroid.getPeakCandidateIndices(zoom=zoom, distBound=distBound)
        centroid.zoom = zoom
        deltaDetFun = self._detection_function(sums, zoom)
        # invalidating non candidate peaks:
        deltaDetFun[~ind_candidates] = 0
        Nft = self.sig_repr_params['fsize']
        deltaAxis = np.concatenate([np.arange(start=0, stop=Nft * zoom // 2),
                                    np.arange(start=-Nft * zoom // 2, stop=0)]) * 1. / zoom
        indMaxDelta = np.argmax(deltaDetFun)
        peakDelta = deltaDetFun[indMaxDelta]
        maxDelta = deltaAxis[indMaxDelta]
        indicePeak = get_indices_peak(sequence=deltaDetFun, ind_max=indMaxDelta,
                                      threshold=threshold)
        if not np.isinf(distBound) and np.any(deltaDetFun[~indicePeak] > threshold * peakDelta):
            maxDelta = None
        return maxDelta

    def identify_deltaT(self, ind_cluster_pts, centroid, threshold=0.8):
        """returns the delay maxDelta in samples that corresponds to the
        largest peak of the cluster defined by the provided cluster index
        """
        return self._identify_deltaT(self._host_sums(ind_cluster_pts), centroid, threshold)

    def _delta_pass(self, slot, centroid, only_centroid):
        frequencies = self.freqs / self.audioObject.samplerate
        with np.errstate(all='ignore'):
            # conjugated v centroid : hence the + in the complex exp
            v1 = np.ascontiguousarray(
                np.exp(1j * 2 * np.pi * centroid.delta * frequencies) * np.sin(centroid.theta),
                dtype=np.complex128)
            maxErrorTheta = self.estim_bound_var_theta(confidence=centroid.confidence,
                                                       u=uVarBound)
        counts = (ctypes.c_long * 2)()
        flat = int(centroid.index_freq) * self._L + int(centroid.index_time)
        check(lib.demix_delta_pass(self._need_ctx('features'), slot, float(centroid.theta),
                                   dptr(v1), float(centroid.confidence), float(maxErrorTheta),
                                   flat, int(only_centroid), counts), "demix_delta_pass")
        self._have_subset = True
        return int(counts[0]), int(counts[1])

    def getTFPointsNearDelta(self, centroid):
        """returns a TF mask which is True if their corresponding value of
        `delta` is close enough to the delta from the `centroid`.  The mask is
        computed on the device into a spare slot, downloaded, and the set of
        points still to classify is left as it was."""
        self._need_ctx('features')
        spare = self.maxclusters - 1
        if spare in self._slots:
            raise ValueError("getTFPointsNearDelta: no spare mask (maxclusters clusters are kept)")
        had = self._have_subset
        keep = self._get_mask(-1) if had else None
        self._delta_pass(spare, centroid, only_centroid=False)
        mask = self._get_mask(spare)
        if had:
            self._set_mask(-1, keep)
        self._have_subset = had
        return mask

    # ---------------------------------------------------------------- features
    def comp_sig_repr(self):
        """Computes the signal representation, stft"""
        if not hasattr(self.audioObject, '_data'):
            self.audioObject._read()
        if self.verbose:
            print("Computing the chosen signal representation:")
        nc = self.audioObject.channels
        if nc != 2:
            raise ValueError("This implementation only deals " +
                             "with stereo audio!")
        self.sig_repr = {}
        # if more than 2 min of signal, take 2 min in the middle
        lengthData = self.audioObject.data.shape[0]
        startData = 0
        endData = lengthData
        oneMinLenData = 60 * self.audioObject.samplerate
        oneMinLenData *= 2
        if lengthData > oneMinLenData:
            startData = (lengthData - oneMinLenData) // 2
            endData = startData + oneMinLenData
        if self.sig_repr_params['tfrepresentation'] == 'stftold':
            for c in range(2):
                self.sig_repr[c], freqs, times = _stft(
                    self.audioObject.data[startData:endData, c],
                    window=np.hanning(self.sig_repr_params['wlen']),
                    hopsize=self.sig_repr_params['hopsize'],
                    nfft=self.sig_repr_params['fsize'],
                    fs=self.audioObject.samplerate, device=self.device)
        else:
            self.tft.computeTransform(self.audioObject.data[startData:endData, 0])
            self.sig_repr[0] = self.tft.transfo
            self.tft.computeTransform(self.audioObject.data[startData:endData, 1])
            self.sig_repr[1] = self.tft.transfo
            freqs = self.tft.freq_stamps
        # keeping the frequencies, not computing them each time
        self.freqs = freqs
        del self.audioObject.data

    def comp_pcafeatures(self):
        """Compute the PCA features and, in the same device call, the planes
        comp_parameters would derive from them (confidence with its energy
        weighting, theta, phi, the variance of theta)."""
        if not hasattr(self, 'X0'):  # never holds: recomputed on every call
            self.comp_sig_repr()
        x0 = np.ascontiguousarray(self.sig_repr[0], dtype=np.complex128)
        x1 = np.ascontiguousarray(self.sig_repr[1], dtype=np.complex128)
        F, N = x0.shape
        nb = int(self.neighbors)
        if nb < 1 or nb > N:
            raise ValueError("DEMIX: neighbors %r outside 1 .. %d frames" % (self.neighbors, N))
        self._free_ctx()
        ctx = ctypes.c_void_p()
        check(lib.demix_create(self.device, F, N, nb, int(self.maxclusters), ctypes.byref(ctx)),
              "demix_create")
        self._ctx = ctx
        self._F, self._L = F, N - nb + 1
        self._slots = []
        self._have_subset = False
        check(lib.demix_features(ctx, dptr(x0), dptr(x1)), "demix_features")
        self.features_ms = last_ms()
        # no need for the signal representation anymore, for now:
        del self.sig_repr

    def comp_parameters(self):
        """The parameterization of the steering vectors

            u_k = [cos(theta_k) sin(theta_k) exp(-j 2 pi f delta_k)]^T

        (confidence[:2] = eps, phiAll, thetaAll, thetaVarAll) is computed by
        comp_pcafeatures' device call; nothing is left to do here."""
        self._need_ctx('features')

    def estim_var_theta(self, confidence):
        maxLim_confidence = 3073.
        thetaVarAll = np.ones_like(confidence)
        indNotZeroConf = np.where(confidence > eps)
        with np.errstate(all='ignore'):
            thetaVarAll[indNotZeroConf[0], indNotZeroConf[1]] = (
                10 ** (confidence[indNotZeroConf[0], indNotZeroConf[1]] / 20.) /
                ((self.neighbors - 1) *
                 (10 ** (confidence[indNotZeroConf[0], indNotZeroConf[1]] / 20.)
                  - 1) ** 2)
                )
        thetaVarAll[confidence >= maxLim_confidence] = 0
        thetaVarAll[confidence <= eps] = np.inf
        return thetaVarAll

    def estim_bound_var_theta(self, confidence, infOrSup='sup', u=2.33):
        minConfidence = 0.
        sigma = np.sqrt(1600. / (self.neighbors - 1.))
        signInfSup = {'inf': 1, 'sup': -1}
        # in place for an array argument, as in the reference
        confidence += signInfSup[infOrSup] * u * sigma
        confidence = np.maximum(confidence, minConfidence)
        confidence = np.atleast_2d(confidence)
        if np.size(confidence) > 1:
            return self.estim_var_theta(confidence)
        else:
            return self.estim_var_theta(confidence)[0, 0]

    def estimDAOBound(self, confidence, confidenceVal=None):
        """computes the max distance between centroid and points"""
        maxErrorTheta = self.estim_bound_var_theta(confidence=confidence, u=uVarBound)
        if confidenceVal is not None:
            thetaVarAll = self.estim_bound_var_theta(confidence=confidenceVal, u=uVarBound)
        else:
            thetaVarAll = self.thetaVarAll
        with np.errstate(all='ignore'):
            return (np.sqrt(thetaVarAll) + np.sqrt(maxErrorTheta)) * uDistBound

    def init_subpts_set(self):
        # setting the "mask" of the points to classify to full
        try:
            check(lib.demix_init_subset(self._need_ctx('confidence')), "demix_init_subset")
        except AttributeError:
            raise AttributeError("no lbd0 in object!")
        self._have_subset = True

    def get_max_confidence_point(self):
        out = np.empty(4)
        check(lib.demix_argmax(self._need_ctx('confidence'), dptr(out)), "demix_argmax")
        flat = int(out[0])
        return TFPoint(demixinstance=self, index_freq=flat // self._L,
                       index_time=flat % self._L, _values=(out[2], out[3], out[1]))

    # -------------------------------------------------------------- refinement
    def reestimate_clusterCentroids(self):
        """reestimate cluster centroids

        considering all the cluster masks, reestimate the centroids,
        discarding the clusters for which there was no well-defined delta.
        """
        if not hasattr(self, 'clusterCentroids'):
            self.comp_clusters()
        # filtering out clusters for which we dont have a correct delay:
        ind_good_cluster = ~np.isnan([c.delta for c in self.clusterCentroids])
        good = np.where(ind_good_cluster)[0]
        self.clusterCentroids = [self.clusterCentroids[n] for n in good]
        self._slots = [self._slots[n] for n in good]
        self._sizes = [self._sizes[n] for n in good]
        # filtering out the Time-Freq points that are in several clusters:
        self.create_exclusive_clusters()
        # adaptive thresholding of clusters; the thresholded masks are not
        # kept: their sums are all the re-estimation reads
        thresholded, sums = self._thresholded_sums()
        # estimation of centroids for each cluster
        for n in range(len(thresholded)):
            if sums[n, 3] != 0:
                with np.errstate(all='ignore'):
                    # normalisation coeff:
                    varP = 1. / sums[n, 0]
                    # weighted mean of thetas, weight is varP/variance
                    theta = varP * sums[n, 1]
                    # confidence of the estimation:
                    varBound = 1. / sums[n, 2]
                    clusterConfidence = confidenceFromVar(varBound, self.neighbors)
                # indexed by the thresholded list's position, as in the reference
                if clusterConfidence > self.clusterCentroids[n].confidence:
                    self.clusterCentroids[n].theta = theta
                    self.clusterCentroids[n].confidence = clusterConfidence

    def create_exclusive_clusters(self):
        """reconfigures the cluster masks such that a Time-Freq point that
        appears in more than one cluster stays in the first that claimed it
        (the running count == 1), then drops the empty clusters."""
        if '_slots_set' not in self.__dict__:
            self.comp_clusters()
        if len(self._slots):
            slots = np.ascontiguousarray(self._slots, dtype=np.int32)
            sizes = (ctypes.c_long * len(self._slots))()
            check(lib.demix_exclusive(self._need_ctx('clusters'), len(self._slots), iptr(slots),
                                      sizes), "demix_exclusive")
            self._sizes = [int(s) for s in sizes]
        else:
            warnings.warn("create_exclusive_clusters: no clusters anymore!")
        self.remove_empty_clusters()

    def get_centroid_distance(self):
        """distance between the centroids"""
        nbClusters = len(self._slots)
        nbFreqs = self.sig_repr_params['fsize'] // 2 + 1
        distanceArray = np.zeros([nbClusters, nbClusters])
        # frequencies vector:
        f = np.arange(0, nbFreqs) * 1. / self.sig_repr_params['fsize']
        for n in range(nbClusters):
            for m in range(n + 1, nbClusters):
                theta = self.clusterCentroids[n].theta
                alpha = self.clusterCentroids[m].theta
                diffDelta = (self.clusterCentroids[n].delta -
                             self.clusterCentroids[m].delta)
                with np.errstate(all='ignore'):
                    d2 = (2. * (1. -
                                np.mean(1. / np.sqrt(2.) *
                                        np.sqrt(1. +
                                                np.cos(2 * alpha) * np.cos(2 * theta) +
                                                np.sin(2 * alpha) * np.sin(2 * theta) *
                                                np.cos(2. * np.pi * f * diffDelta)),
                                        axis=0)))
                    distanceArray[n, m] = np.sqrt(d2)
        return distanceArray

    def _confidence_thresholds(self):
        distanceArray = self.get_centroid_distance()
        nbClusters = len(self._slots)
        confidenceThreshold = np.zeros(nbClusters)
        distTocluster = np.ones(nbClusters) * 2
        for n in range(nbClusters):
            clustersMinusN = list(range(nbClusters))
            clustersMinusN.remove(n)
            for m in clustersMinusN:
                dist_n_m = np.copy(distanceArray[min(n, m), max(n, m)])
                # max erreurs sur l'estimation des centroids:
                dist_centroid_n = self.estimDAOBound(
                    confidence=self.clusterCentroids[n].confidence, confidenceVal=np.inf)
                dist_centroid_m = self.estimDAOBound(
                    confidence=self.clusterCentroids[m].confidence, confidenceVal=np.inf)
                dist_n_m -= (dist_centroid_n + dist_centroid_m)
                dist_n_m = max(dist_n_m, 0.)
                distTocluster[n] = min(dist_n_m, distTocluster[n])
            # estimation of threshold
            confidenceThreshold[n] = confidenceFromVar((distTocluster[n] / 2) ** 2,
                                                       self.neighbors)
        return confidenceThreshold

    def _thresholded_sums(self):
        """The thresholded clusters as (slot, threshold) pairs and their sums
        [n, 4] (sum 1/var, sum theta/var, sum 1/varBound, count).  Like the
        reference's adaptive_thresholding_clusters, removes the clusters that
        are empty from self.clusters, not from the list it returns."""
        confidenceThreshold = self._confidence_thresholds()
        thresholded = list(zip(self._slots, confidenceThreshold))
        sums = np.zeros((len(thresholded), 4))
        if len(thresholded):
            slots = np.ascontiguousarray(self._slots, dtype=np.int32)
            thr = np.ascontiguousarray(confidenceThreshold, dtype=np.float64)
            check(lib.demix_cluster_sums(self._need_ctx('clusters'), len(thresholded), iptr(slots),
                                         dptr(thr), dptr(sums)), "demix_cluster_sums")
        # to avoid errors when considering empty clusters...
        self.remove_empty_clusters()
        return thresholded, sums

    def adaptive_thresholding_clusters(self):
        """compute for each cluster in self.clusters a threshold depending
        on the other clusters, in order to keep only those points in cluster
        that are close to the actual centroid, but not close to centroids of
        other clusters.

        The returned clusters are the original clusters thresholded
        (downloaded masks; the re-estimation itself reads their sums on the
        device).
        """
        confidenceThreshold = self._confidence_thresholds()
        confidence = self.confidence if len(self._slots) else None
        thresholdedClusters = [self._get_mask(s) * (confidence >= confidenceThreshold[n])
                               for n, s in enumerate(self._slots)]
        self.remove_empty_clusters()
        return thresholdedClusters

    def keepBestClusters(self, nsources=None):
        if nsources is None:
            nsources = self.nsources
        if nsources is None:
            raise AttributeError('The nb of sources is not provided.')
        nclusters = len(self._slots)
        if nclusters < nsources:
            warnings.warn("The number of clusters %d" % nclusters +
                          "is different from the required\nnumber of sources" +
                          " %d." % nsources)
        else:
            confidences = [cc.confidence for cc in self.clusterCentroids]
            sortedIndices = np.argsort(confidences)
            # indices of increasing values sorted: read upside down:
            best = sortedIndices[:-(nsources + 1):-1]
            self.clusterCentroids = [self.clusterCentroids[n] for n in best]
            self._slots = [self._slots[n] for n in best]
            self._sizes = [self._sizes[n] for n in best]

    def remove_empty_clusters(self):
        clustersizes = np.array(self._sizes, dtype=int)
        if self.verbose > 1:
            print("remove_empty_clusters")
            print("    cluster sizes:", clustersizes)
            print("    Removing", np.sum(clustersizes == 0), "clusters")
        keep = np.where(clustersizes > 0)[0]
        self._slots = [self._slots[n] for n in keep]
        self._sizes = [self._sizes[n] for n in keep]
        self.clusterCentroids = [self.clusterCentroids[n] for n in keep]

    def remove_weak_clusters(self, distanceArray=None, clusterDistBounds=None):
        raise NotImplementedError("DEMIX.remove_weak_clusters (nsources=None) is not implemented")

    def spatial_filtering(self):
        raise NotImplementedError(
            "DEMIX.spatial_filtering is not implemented; build the filters from "
            "steeringVectorsFromCentroids() and apply them with tftransforms.stft.filter_stft")

    def steeringVectorsFromCentroids(self):
        """Generates the steering vectors a(p,f,c) for source p,
        (reduced) freq f and channel c:

          a[p,f,0] = cos(theta_p)
          a[p,f,1] = sin(theta_p) exp(- 2 j pi f delta_p)
        """
        if not hasattr(self, "freqs"):
            self.comp_sig_repr()
        thetas = [cc.theta for cc in self.clusterCentroids]
        deltas = [cc.delta for cc in self.clusterCentroids]
        # frequencies in reduced form (from 0 to 1/2)
        freqs = self.freqs * 1. / self.audioObject.samplerate
        nsrc = len(self.clusterCentroids)
        A = np.zeros([nsrc, self.freqs.size, self.audioObject.channels], dtype=complex)
        if nsrc > 0:
            # left channel:
            A[:, :, 0] = np.vstack(np.cos(thetas))
            # right channel:
            A[:, :, 1] = (np.vstack(np.sin(thetas)) *
                          np.exp(- 1j * 2. * np.pi * np.outer(deltas, freqs)))
        else:
            warnings.warn("Caution: the number of sources is %d." % nsrc)
        return A


class TFPoint(object):
    def __init__(self, demixinstance=None, thetaphidelta=None,
                 index_scale=0, index_freq=0, index_time=0,
                 verbose=2, _values=None):
        if demixinstance is None and thetaphidelta is not None:
            self.theta = thetaphidelta[0]
            self.phi = thetaphidelta[1]
            self.delta = thetaphidelta[2]
            self.confidence = 100.
            self.index_scale = index_scale  # for future integration
            self.index_freq = index_freq
            self.index_time = index_time
            self.frequency = 0.
        elif demixinstance is not None:
            if _values is None:
                # three planes cross to the host for three numbers: the
                # clustering loop passes the values of its device argmax
                _values = (demixinstance.thetaAll[index_freq, index_time],
                           demixinstance.phiAll[index_freq, index_time],
                           demixinstance.confidence[index_freq, index_time])
            self.theta, self.phi, self.confidence = (np.float64(v) for v in _values)
            self.frequency = (
                index_freq * 1. / demixinstance.sig_repr_params['fsize'])
            self.index_scale = index_scale  # for future integration
            self.index_freq = index_freq
            self.index_time = index_time
            # to be able to use general purpose methods like:
            #    estim_bound_var_theta
            self.demixInst = demixinstance
        else:
            print("TFPoint: generating dummy TFPoint")
        self.verbose = verbose

    def estimDeltaPhi(self):
        """Estimates a bound on the distance
        confidence interval, in samples, to the TFpoint delta
        """
        with np.errstate(all='ignore'):
            dmax = np.sqrt(
                self.demixInst.estim_bound_var_theta(
                    confidence=self.confidence,
                    infOrSup='sup',
                    u=uVarBound)
                ) * uDistBound
            cos_ds = (dmax ** 2 - 2) ** 2 / 2 - 1  # where does this come from...
            if np.arccos(cos_ds) <= min(2 * self.theta, np.pi - 2 * self.theta):
                alpha = 0.5 * np.arccos(np.cos(2 * self.theta) / cos_ds)
                deltaPhi = np.arccos(
                    (cos_ds - np.cos(2 * self.theta) * np.cos(2 * alpha)) /
                    (np.sin(2 * self.theta) * np.sin(2 * alpha))
                    )
                return deltaPhi / (2 * np.pi * self.frequency)
            else:
                return np.inf

    def getPeakCandidateIndices(self, zoom=1, distBound=None):
        """computes the indices of compatible delta bins"""
        if distBound is None:
            _, distBound = self.demixInst.getTFpointsNearTheta_OneScale(centroid_tfpoint=self)
        Nft = self.demixInst.sig_repr_params['fsize']
        kmax = np.floor((2 * np.pi * self.frequency * Nft / 2 - np.abs(self.phi)) /
                        (2 * np.pi))
        kmax = np.maximum(kmax, 0)
        ks = np.arange(-kmax, kmax + 1)
        centroidDeltas = (- self.phi + 2 * np.pi * ks) / (2 * np.pi * self.frequency)
        deltaXiFFTmin = - (Nft * zoom // 2 - 1)
        deltaXiFFTmax = (Nft * zoom // 2)
        infBounds = np.zeros(len(ks))
        supBounds = np.zeros(len(ks))
        bound1 = np.ceil((centroidDeltas - distBound) * zoom)
        bound2 = np.floor((centroidDeltas + distBound) * zoom)
        bound1 = np.maximum(deltaXiFFTmin, bound1)
        bound1 = np.minimum(deltaXiFFTmax, bound1)
        bound2 = np.maximum(deltaXiFFTmin, bound2)
        bound2 = np.minimum(deltaXiFFTmax, bound2)
        infBounds[bound1 >= 0] = bound1[bound1 >= 0]
        infBounds[bound1 < 0] = bound1[bound1 < 0] + deltaXiFFTmax - deltaXiFFTmin + 1
        supBounds[bound2 >= 0] = bound2[bound2 >= 0]
        supBounds[bound2 < 0] = bound2[bound2 < 0] + deltaXiFFTmax - deltaXiFFTmin + 1
        if np.isinf(distBound):
            # return a True vector for all time bins:
            self.indices_candidates = np.ones(Nft * zoom, dtype=bool)
        else:
            self.indices_candidates = np.zeros(Nft * zoom, dtype=bool)
            for n in range(len(ks)):
                if infBounds[n] <= supBounds[n]:
                    self.indices_candidates[int(infBounds[n]):int(supBounds[n] + 1)] = True
                else:
                    self.indices_candidates[int(infBounds[n]):] = True
                    self.indices_candidates[:int(supBounds[n] + 1)] = True
        return self.indices_candidates

    def clusterDistBound(self):
        raise NotImplementedError("TFPoint.clusterDistBound (nsources=None) is not implemented")

    def __str__(self):
        return ("[confidence: " + str(self.confidence) +
                ", delta: " + str(getattr(self, 'delta', None)) + ", " +
                "phi :" + str(self.phi) +
                ", theta: " + str(self.theta) + ", " +
                "freq : " + str(self.frequency) + "]")

    def __repr__(self):
        return self.__str__()
