"""NumPy restatement of the reference's demixTF.py (DEMIX, TFPoint), line by
line with its quirks, plus the decision margins that make an exact comparison
of masks legitimate.  tests/test_demix_ref_golden.py pins it
to the reference's own numbers (tests/golden/demix_<case>.npz).

Differences from the reference's text: the stereo samples and the sample rate
are given as arrays (no AudioObject), 'stft' only, `nsources=None` stops after
comp_clusters (remove_weak_clusters is not restated), nothing is printed.
`pca='fft'` sums the PCA windows with scipy's fftconvolve as the reference
does, `pca='direct'` in ascending frame order as the device does
(tests/sigtools_ref.py).

Margins.  Every comparison that decides a mask is recorded with its relative
gap |lhs - rhs| / max(|rhs|, TINY):
  * theta test   |thetaAll - theta_c| < distBound                (per round)
  * delta test   dist < distBound of getTFPointsNearDelta, and, where the
                 test would pass without it, the veto confidence_c < confidence
  * threshold    confidence >= confidenceThreshold[n], inside cluster n
  * argmax       (max - largest value below it) / max; exact ties are counted
                 in `argmax_ties` with the tied value.
A comparison against an infinite or NaN side, or against a bound of 0 (no
distance is below it), cannot flip and has margin inf.  `point_margin` is the
minimum over the rounds of the delta test's margins at each point.
"""
import warnings

import numpy as np

import sigtools_ref

eps = 1e-10
uVarBound = 2.33
uDistBound = 2.33
TINY = 1e-300
MARGIN_MIN = 1e-9


def decibel(val):
    return 20. * np.log10(val)


def invdb(dbval):
    return 10. ** (dbval / 20.)


def get_indices_peak(sequence, ind_max, threshold=0.8):
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
    alpha = ((2 * variance * (neighbors - 1) + 1 + np.sqrt(1 + 4 * variance * (neighbors - 1)))
             / (2 * variance * (neighbors - 1)))
    return 20 * np.log10(alpha)


def nextpow2(i):
    n = 2
    while n < i:
        n = n * 2
    return n


def sqrt_blackmanharris(M):
    import scipy.signal as spsig
    return np.sqrt(spsig.windows.blackmanharris(M))


def prin_comp_2d_fft(X0, X1, neighborNb):
    """signalTools.py:26-118 with its fftconvolve window sums."""
    import scipy.signal as spsig
    F, N = X0.shape
    lenCov = N - neighborNb + 1
    ones = np.ones(neighborNb)
    cov0_2 = np.zeros([F, lenCov])
    cov1_2 = np.zeros([F, lenCov])
    cov01 = np.zeros([F, lenCov], dtype=complex)
    for f in range(F):
        cov0_2[f] = np.abs(spsig.fftconvolve(in1=np.abs(X0[f]) ** 2, in2=ones, mode='valid')) / (neighborNb - 1.)
        cov1_2[f] = np.abs(spsig.fftconvolve(in1=np.abs(X1[f]) ** 2, in2=ones, mode='valid')) / (neighborNb - 1.)
        cov01[f] = spsig.fftconvolve(in1=X0[f] * np.conj(X1[f]), in2=ones, mode='valid') / (neighborNb - 1.)
    traSig = cov0_2 + cov1_2
    detSig = cov0_2 * cov1_2 - np.abs(cov01) ** 2
    delta = np.sqrt(traSig ** 2 - 4 * detSig)
    lambdaM = .5 * (traSig + delta)
    lambdam = .5 * (traSig - delta)
    vM = np.zeros([2, F, lenCov], dtype=complex)
    den = np.sqrt(np.abs(cov01) ** 2 + np.abs(lambdaM - cov0_2) ** 2)
    vM[0] = cov01 / den
    vM[1] = (lambdaM - cov0_2) / den
    vM[0][den == 0] = 1
    vM[1][den == 0] = 0
    return lambdaM, lambdam, vM


def _gap(lhs, rhs):
    """Relative gap of a comparison lhs ? rhs; inf where it cannot flip."""
    lhs, rhs = np.broadcast_arrays(np.asarray(lhs, dtype=float), np.asarray(rhs, dtype=float))
    g = np.full(lhs.shape, np.inf)
    ok = np.isfinite(lhs) & np.isfinite(rhs)
    g[ok] = np.abs(lhs[ok] - rhs[ok]) / np.maximum(np.abs(rhs[ok]), TINY)
    return g


class TFPoint(object):
    def __init__(self, demixinstance, index_freq=0, index_time=0):
        self.theta = demixinstance.thetaAll[index_freq, index_time]
        self.phi = demixinstance.phiAll[index_freq, index_time]
        self.confidence = demixinstance.confidence[index_freq, index_time]
        self.frequency = index_freq * 1. / demixinstance.fsize
        self.index_freq = index_freq
        self.index_time = index_time
        self.demixInst = demixinstance

    def estimDeltaPhi(self):
        dmax = np.sqrt(self.demixInst.estim_bound_var_theta(
            confidence=self.confidence, infOrSup='sup', u=uVarBound)) * uDistBound
        cos_ds = (dmax ** 2 - 2) ** 2 / 2 - 1
        if np.arccos(cos_ds) <= min(2 * self.theta, np.pi - 2 * self.theta):
            alpha = 0.5 * np.arccos(np.cos(2 * self.theta) / cos_ds)
            deltaPhi = np.arccos((cos_ds - np.cos(2 * self.theta) * np.cos(2 * alpha)) /
                                 (np.sin(2 * self.theta) * np.sin(2 * alpha)))
            return deltaPhi / (2 * np.pi * self.frequency)
        else:
            return np.inf

    def getPeakCandidateIndices(self, zoom=1, distBound=None):
        Nft = self.demixInst.fsize
        kmax = np.floor((2 * np.pi * self.frequency * Nft / 2 - np.abs(self.phi)) / (2 * np.pi))
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


class RefDEMIX(object):
    def __init__(self, data, samplerate, nsources=2, wlen=2048, hopsize=1024, neighbors=20,
                 maxclusters=100, winFunc=sqrt_blackmanharris, pca='fft'):
        self.nsources = nsources
        if nsources is None:
            self.maxclusters = maxclusters
        else:
            self.maxclusters = np.maximum(maxclusters, self.nsources * 10)
        self.neighbors = neighbors
        self.data = np.asarray(data, dtype=float)
        self.samplerate = samplerate
        self.wlen = wlen
        self.fsize = nextpow2(wlen)
        self.hopfactor = 1. * hopsize / wlen
        self.fthop = int(self.fsize * self.hopfactor)
        self.window = winFunc(self.fsize)
        self.pca = pca
        self.rounds = []
        self.margins = {'theta': np.inf, 'delta': np.inf, 'threshold': np.inf, 'argmax': np.inf}
        self.argmax_ties = []

    # ------------------------------------------------------------- features
    def comp_sig_repr(self):
        import fasst_ref
        if self.data.ndim != 2 or self.data.shape[1] != 2:
            raise ValueError("This implementation only deals with stereo audio!")
        lengthData = self.data.shape[0]
        startData = 0
        endData = lengthData
        oneMinLenData = 60 * self.samplerate
        oneMinLenData *= 2
        if lengthData > oneMinLenData:
            startData = (lengthData - oneMinLenData) // 2
            endData = startData + oneMinLenData
        self.sig_repr = {}
        for c in range(2):
            self.sig_repr[c] = fasst_ref.stft(self.data[startData:endData, c], self.window,
                                              self.fthop, self.fsize)
        self.freqs = np.arange(self.fsize // 2 + 1) / np.double(self.fsize) * self.samplerate

    def comp_pcafeatures(self):
        self.comp_sig_repr()  # hasattr(self, 'X0') never holds
        with np.errstate(all='ignore'):
            if self.pca == 'fft':
                lbd0, lbd1, self.egv0 = prin_comp_2d_fft(self.sig_repr[0], self.sig_repr[1],
                                                         self.neighbors)
            else:
                lbd0, lbd1, self.egv0, _ = sigtools_ref.prin_comp_2d(
                    self.sig_repr[0], self.sig_repr[1], self.neighbors)
            self.confidence = 20. * np.log10(lbd0 / np.maximum(lbd1, eps))
        self.lbd = (np.array(lbd0), np.array(lbd1))  # kept for the tests' error propagation
        self.confidence[np.isnan(self.confidence)] = 0.
        start = self.neighbors // 2
        energy = np.mean(np.array(list(self.sig_repr.values())) ** 2,
                         axis=0)[:, start:start + self.confidence.shape[1]]
        self.confidence[energy < energy.max() * 1e-6] = 0.
        del self.sig_repr

    def comp_parameters(self):
        self.confidence[:2, :] = eps
        with np.errstate(all='ignore'):
            self.phiAll = np.angle(self.egv0[1] / self.egv0[0])
            self.thetaAll = np.arctan(np.abs(self.egv0[1]) / np.abs(self.egv0[0]))
        self.thetaVarAll = self.estim_var_theta(confidence=self.confidence)
        del self.egv0

    def estim_var_theta(self, confidence):
        maxLim_confidence = 3073.
        thetaVarAll = np.ones_like(confidence)
        ind = np.where(confidence > eps)
        with np.errstate(all='ignore'):
            thetaVarAll[ind[0], ind[1]] = (
                10 ** (confidence[ind[0], ind[1]] / 20.) /
                ((self.neighbors - 1) * (10 ** (confidence[ind[0], ind[1]] / 20.) - 1) ** 2))
        thetaVarAll[confidence >= maxLim_confidence] = 0
        thetaVarAll[confidence <= eps] = np.inf
        return thetaVarAll

    def estim_bound_var_theta(self, confidence, infOrSup='sup', u=2.33):
        minConfidence = 0.
        sigma = np.sqrt(1600. / (self.neighbors - 1.))
        signInfSup = {'inf': 1, 'sup': -1}
        confidence += signInfSup[infOrSup] * u * sigma
        confidence = np.maximum(confidence, minConfidence)
        confidence = np.atleast_2d(confidence)
        if np.size(confidence) > 1:
            return self.estim_var_theta(confidence)
        else:
            return self.estim_var_theta(confidence)[0, 0]

    def estimDAOBound(self, confidence, confidenceVal=None):
        maxErrorTheta = self.estim_bound_var_theta(confidence=confidence, u=uVarBound)
        if confidenceVal is not None:
            thetaVarAll = self.estim_bound_var_theta(confidence=confidenceVal, u=uVarBound)
        else:
            thetaVarAll = self.thetaVarAll
        return (np.sqrt(thetaVarAll) + np.sqrt(maxErrorTheta)) * uDistBound

    # ----------------------------------------------------------- clustering
    def init_subpts_set(self):
        self.subTFpointSet = np.ones(self.confidence.shape, dtype=bool)

    def get_max_confidence_point(self):
        tmpConfidence = np.copy(self.confidence)
        tmpConfidence[~self.subTFpointSet] = 0
        flat = tmpConfidence.argmax()
        vmax = tmpConfidence.flat[flat]
        below = tmpConfidence[tmpConfidence < vmax]
        ties = int(np.sum(tmpConfidence == vmax))
        if ties > 1:
            self.argmax_ties.append((len(self.rounds), float(vmax), ties))
        if below.size and vmax > 0:
            self.margins['argmax'] = min(self.margins['argmax'],
                                         float((vmax - below.max()) / max(vmax, TINY)))
        index = np.unravel_index(flat, tmpConfidence.shape)
        return TFPoint(self, index_freq=int(index[0]), index_time=int(index[1]))

    def getTFpointsNearTheta_OneScale(self, centroid_tfpoint):
        with np.errstate(all='ignore'):
            dist = np.abs(self.thetaAll - centroid_tfpoint.theta)
            distBound = np.sqrt(self.estim_bound_var_theta(
                centroid_tfpoint.confidence, infOrSup='sup', u=uVarBound)) * uDistBound
            distBound = 1 / 2. * np.arccos(((distBound ** 2 - 2) ** 2) / 2. - 1)
            g = _gap(dist, distBound)[self.subTFpointSet]
            if g.size:
                self.margins['theta'] = min(self.margins['theta'], float(g.min()))
            return (dist < distBound) * self.subTFpointSet, distBound

    def compute_temporal(self, ind_cluster_pts, zoom):
        with np.errstate(all='ignore'):
            thetaVars = np.copy(self.thetaVarAll)
            thetaVars[thetaVars == 0] = eps
            y = (1 / thetaVars) * np.exp(1j * self.phiAll)
            thetaVars[~ind_cluster_pts] = np.inf
            y[~ind_cluster_pts] = 0
            normalisation = np.sum((1 / thetaVars), axis=1)
            normalisation[normalisation == 0] = eps
            return np.fft.irfft(y.sum(axis=1) / normalisation, n=self.fsize * zoom)

    def identify_deltaT(self, ind_cluster_pts, centroid, threshold=0.8):
        with np.errstate(all='ignore'):
            distBound = centroid.estimDeltaPhi()
            nbMaxSamples = 2 ** 7
            zoomMax = 2 ** 4
            if distBound != np.inf:
                zoom = 2 ** np.ceil(np.log2(nbMaxSamples / 2 * distBound))
                zoom = max(1, zoom)
                zoom = min(zoom, zoomMax)
                zoom = int(zoom)
            else:
                zoom = 1
            self.last_zoom = zoom
            ind_candidates = centroid.getPeakCandidateIndices(zoom=zoom, distBound=distBound)
        deltaDetFun = self.compute_temporal(ind_cluster_pts=ind_cluster_pts, zoom=zoom)
        deltaDetFun[~ind_candidates] = 0
        Nft = self.fsize
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

    def getTFPointsNearDelta(self, centroid):
        frequencies = self.freqs / self.samplerate
        with np.errstate(all='ignore'):
            u0 = np.cos(self.thetaAll)
            u1 = np.sin(self.thetaAll) * np.exp(1j * self.phiAll)
            v_centroid = np.vstack([
                np.ones(self.freqs.size) * np.cos(centroid.theta),
                np.exp(1j * 2 * np.pi * centroid.delta * frequencies) * np.sin(centroid.theta)])
            dist = np.sqrt(2 * (1 - np.abs(u0 * np.vstack(v_centroid[0]) +
                                           u1 * np.vstack(v_centroid[1]))))
            distBound = self.estimDAOBound(confidence=centroid.confidence)
            # margins: the distance test, and the veto where it decides
            g = _gap(dist, distBound)
            veto = centroid.confidence < self.confidence
            gv = _gap(self.confidence, centroid.confidence)
            decides = dist < distBound
            g = np.where(veto, np.where(decides, gv, np.inf), np.minimum(g, np.where(decides, gv, np.inf)))
            g[centroid.index_freq, centroid.index_time] = np.inf
            self.point_margin = np.minimum(self.point_margin, g)
            self.margins['delta'] = min(self.margins['delta'], float(g.min()))
            distBound[veto] = 0
            ind_cluster_pts = (dist < distBound)
        ind_cluster_pts[centroid.index_freq, centroid.index_time] = True
        return ind_cluster_pts

    def comp_clusters(self, threshold=0.8):
        self.comp_pcafeatures()
        self.comp_parameters()
        self.init_subpts_set()
        self.point_margin = np.full(self.confidence.shape, np.inf)
        self.clusterCentroids = []
        self.clusters = []
        self.rounds = []
        nbRemainingPoints = self.subTFpointSet.sum()
        while nbRemainingPoints and len(self.clusters) < self.maxclusters:
            c = self.get_max_confidence_point()
            self.clusterCentroids.append(c)
            ind_cluster_theta_pts, distBound = self.getTFpointsNearTheta_OneScale(c)
            maxDelta = self.identify_deltaT(ind_cluster_pts=ind_cluster_theta_pts, centroid=c,
                                            threshold=threshold)
            if maxDelta is not None:
                c.delta = maxDelta
                ind_cluster_theta_pts = self.getTFPointsNearDelta(centroid=c)
            else:
                c.delta = np.nan
                ind_cluster_theta_pts = ind_cluster_theta_pts * False
                ind_cluster_theta_pts[c.index_freq, c.index_time] = True
            self.clusters.append(ind_cluster_theta_pts)
            self.subTFpointSet *= (~ind_cluster_theta_pts)
            nbRemainingPoints = self.subTFpointSet.sum()
            self.rounds.append(dict(
                index=c.index_freq * self.confidence.shape[1] + c.index_time, theta=c.theta,
                phi=c.phi, confidence=c.confidence, delta=c.delta, zoom=self.last_zoom,
                size=int(ind_cluster_theta_pts.sum()), remaining=int(nbRemainingPoints)))

    # ----------------------------------------------------------- refinement
    def refine_clusters(self):
        self.reestimate_clusterCentroids()
        if self.nsources is not None:
            self.keepBestClusters()
        else:
            raise NotImplementedError("nsources=None: remove_weak_clusters is not restated")
        self.reestimate_clusterCentroids()

    def reestimate_clusterCentroids(self):
        if not hasattr(self, 'clusterCentroids'):
            self.comp_clusters()
        ind_good_cluster = ~np.isnan([c.delta for c in self.clusterCentroids])
        self.clusterCentroids = [self.clusterCentroids[n] for n in np.where(ind_good_cluster)[0]]
        self.clusters = [self.clusters[n] for n in np.where(ind_good_cluster)[0]]
        self.create_exclusive_clusters()
        thresholdedClusters = self.adaptive_thresholding_clusters()
        for n, cluster in enumerate(thresholdedClusters):
            if cluster.sum() != 0:
                confidences = self.confidence[cluster]
                thetas = self.thetaAll[cluster]
                variances = self.thetaVarAll[cluster]
                with np.errstate(all='ignore'):
                    varBounds = self.estim_bound_var_theta(confidence=confidences, infOrSup='sup',
                                                           u=uVarBound)
                    varP = 1. / (np.sum(1. / variances))
                    theta = varP * np.sum(thetas / variances)
                    varBound = 1. / np.sum(1. / varBounds)
                    clusterConfidence = confidenceFromVar(varBound, self.neighbors)
                if clusterConfidence > self.clusterCentroids[n].confidence:
                    self.clusterCentroids[n].theta = theta
                    self.clusterCentroids[n].confidence = clusterConfidence

    def create_exclusive_clusters(self):
        if len(self.clusters):
            maskOnlyOneCluster = np.array(self.clusters[0], dtype=int)
        else:
            warnings.warn("create_exclusive_clusters: no clusters anymore!")
        for clustern, cluster in enumerate(self.clusters[1:]):
            maskOnlyOneCluster += self.clusters[clustern + 1]
            cluster *= (maskOnlyOneCluster == 1)
        self.remove_empty_clusters()

    def get_centroid_distance(self):
        nbClusters = len(self.clusters)
        nbFreqs = self.fsize // 2 + 1
        distanceArray = np.zeros([nbClusters, nbClusters])
        f = np.arange(0, nbFreqs) * 1. / self.fsize
        for n in range(nbClusters):
            for m in range(n + 1, nbClusters):
                theta = self.clusterCentroids[n].theta
                alpha = self.clusterCentroids[m].theta
                diffDelta = self.clusterCentroids[n].delta - self.clusterCentroids[m].delta
                with np.errstate(all='ignore'):
                    d2 = (2. * (1. - np.mean(
                        1. / np.sqrt(2.) * np.sqrt(1. + np.cos(2 * alpha) * np.cos(2 * theta) +
                                                   np.sin(2 * alpha) * np.sin(2 * theta) *
                                                   np.cos(2. * np.pi * f * diffDelta)), axis=0)))
                    distanceArray[n, m] = np.sqrt(d2)
        return distanceArray

    def confidence_thresholds(self):
        """The thresholds of adaptive_thresholding_clusters (its host part)."""
        distanceArray = self.get_centroid_distance()
        nbClusters = len(self.clusters)
        confidenceThreshold = np.zeros(nbClusters)
        distTocluster = np.ones(nbClusters) * 2
        for n in range(nbClusters):
            clustersMinusN = list(range(nbClusters))
            clustersMinusN.remove(n)
            for m in clustersMinusN:
                dist_n_m = np.copy(distanceArray[min(n, m), max(n, m)])
                dist_centroid_n = self.estimDAOBound(
                    confidence=self.clusterCentroids[n].confidence, confidenceVal=np.inf)
                dist_centroid_m = self.estimDAOBound(
                    confidence=self.clusterCentroids[m].confidence, confidenceVal=np.inf)
                dist_n_m -= (dist_centroid_n + dist_centroid_m)
                dist_n_m = max(dist_n_m, 0.)
                distTocluster[n] = min(dist_n_m, distTocluster[n])
            with np.errstate(all='ignore'):
                confidenceThreshold[n] = confidenceFromVar((distTocluster[n] / 2) ** 2,
                                                           self.neighbors)
        return confidenceThreshold

    def adaptive_thresholding_clusters(self):
        confidenceThreshold = self.confidence_thresholds()
        thresholdedClusters = []
        for n in range(len(self.clusters)):
            g = _gap(self.confidence, confidenceThreshold[n])[self.clusters[n]]
            if g.size:
                self.margins['threshold'] = min(self.margins['threshold'], float(g.min()))
            thresholdedClusters.append(self.clusters[n] * (self.confidence >= confidenceThreshold[n]))
        self.remove_empty_clusters()
        return thresholdedClusters

    def keepBestClusters(self, nsources=None):
        if nsources is None:
            nsources = self.nsources
        if nsources is None:
            raise AttributeError('The nb of sources is not provided.')
        nclusters = len(self.clusters)
        if nclusters < nsources:
            warnings.warn("The number of clusters %d" % nclusters +
                          "is different from the required\nnumber of sources" + " %d." % nsources)
        else:
            confidences = [cc.confidence for cc in self.clusterCentroids]
            sortedIndices = np.argsort(confidences)
            self.clusterCentroids = [self.clusterCentroids[n]
                                     for n in sortedIndices[:-(nsources + 1):-1]]
            self.clusters = [self.clusters[n] for n in sortedIndices[:-(nsources + 1):-1]]

    def remove_empty_clusters(self):
        clustersizes = np.array([c.sum() for c in self.clusters])
        self.clusters = [self.clusters[n] for n in np.where(clustersizes > 0)[0]]
        self.clusterCentroids = [self.clusterCentroids[n] for n in np.where(clustersizes > 0)[0]]

    def steeringVectorsFromCentroids(self):
        thetas = [cc.theta for cc in self.clusterCentroids]
        deltas = [cc.delta for cc in self.clusterCentroids]
        freqs = self.freqs * 1. / self.samplerate
        nsrc = len(self.clusterCentroids)
        A = np.zeros([nsrc, self.freqs.size, 2], dtype=complex)
        if nsrc > 0:
            A[:, :, 0] = np.vstack(np.cos(thetas))
            A[:, :, 1] = (np.vstack(np.sin(thetas)) *
                          np.exp(- 1j * 2. * np.pi * np.outer(deltas, freqs)))
        else:
            warnings.warn("Caution: the number of sources is %d." % nsrc)
        return A


# -------------------------------------------------------------------- cases
# fixture case -> constructor arguments (tests/golden/make_golden_demix.py)
CASES = {
    'demix_a': dict(nsources=3, wlen=128, hopsize=64, neighbors=5, winFunc=np.hanning),
    'demix_b': dict(nsources=2, wlen=256, hopsize=64, neighbors=20),
}
FS = 8000


def _band_noise(rs, n, lo, hi):
    """White noise limited to the band [lo, hi) (fractions of the sample rate)."""
    X = np.fft.rfft(rs.randn(n))
    f = np.arange(X.size) / float(n)
    X[(f < lo) | (f >= hi)] = 0
    x = np.fft.irfft(X, n)
    return x / np.abs(x).max()


def _delay(x, d):
    """x delayed by the integer d (circular; negative advances)."""
    return np.roll(x, d)


def mixture(sources, thetas, delays, noise, seed, n):
    """Stereo mixture: channel 0 = sum cos(theta) s, channel 1 = sum sin(theta)
    s delayed by `delays` samples, plus white noise of amplitude `noise`."""
    rs = np.random.RandomState(seed)
    x = np.zeros((n, 2))
    for s, th, d in zip(sources, thetas, delays):
        x[:, 0] += np.cos(th) * s
        x[:, 1] += np.sin(th) * _delay(s, d)
    return x + noise * rs.randn(n, 2)


def case_signal(name):
    """The int16 stereo samples of a fixture case."""
    n = 2 * FS
    if name == 'demix_a':
        rs = np.random.RandomState(11)
        t = np.arange(n) / float(FS)
        env = lambda a, b: ((t >= a) & (t < b)).astype(float)
        srcs = [_band_noise(rs, n, 0.03, 0.17) * env(0.0, 1.2),
                _band_noise(rs, n, 0.12, 0.33) * env(0.5, 2.0),
                _band_noise(rs, n, 0.25, 0.47) * env(0.2, 1.7)]
        x = mixture(srcs, [0.35, 0.8, 1.2], [0, 3, -2], 1e-3, 12, n)
    elif name == 'demix_b':
        n = 3 * FS // 2
        rs = np.random.RandomState(21)
        t = np.arange(n) / float(FS)
        env = lambda a, b: ((t >= a) & (t < b)).astype(float)
        srcs = [_band_noise(rs, n, 0.02, 0.30) * env(0.0, 1.1),
                _band_noise(rs, n, 0.20, 0.48) * env(0.4, 1.5)]
        x = mixture(srcs, [0.5, 1.1], [2, -5], 3e-3, 22, n)
    else:
        raise ValueError(name)
    return np.round(x / np.abs(x).max() * 30000).astype(np.int16)


def read_scaled(samples):
    """audioObject.py:112-127."""
    return samples / np.maximum(1.1 * np.abs(samples).max(), 1e-10)


def live_mixture(n, seed, silent_second=False, fs=FS):
    """Seeded synthetic stereo mixture of three delayed band noises, float."""
    rs = np.random.RandomState(seed)
    srcs = [_band_noise(rs, n, 0.02, 0.2), _band_noise(rs, n, 0.15, 0.35),
            _band_noise(rs, n, 0.3, 0.49)]
    x = mixture(srcs, [0.3, 0.8, 1.25], [0, 3, -2], 2e-3, seed + 1, n)
    if silent_second:
        x[:, 1] = 0
    return x / (1.1 * np.abs(x).max())


def run_case(data, fs, stop_after_clusters=False, **kw):
    """Run the restatement; returns the object and a dict of recorded results
    (the layout of the fixtures)."""
    d = RefDEMIX(data, fs, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d.comp_clusters()
        out = dict(confidence=d.confidence.copy(), thetaAll=d.thetaAll.copy(),
                   phiAll=d.phiAll.copy(), thetaVarAll=d.thetaVarAll.copy())
        for k in ('index', 'theta', 'phi', 'confidence', 'delta', 'zoom', 'size', 'remaining'):
            out['round_' + k] = np.array([r[k] for r in d.rounds])
        out['clusters'] = np.packbits(np.array(d.clusters).reshape(len(d.clusters), -1), axis=1)
        out['subTFpointSet'] = d.subTFpointSet.copy()
        out['lbd0'], out['lbd1'] = d.lbd
        if not stop_after_clusters and d.nsources is not None:
            d.refine_clusters()
            out['ref_theta'] = np.array([c.theta for c in d.clusterCentroids])
            out['ref_delta'] = np.array([c.delta for c in d.clusterCentroids])
            out['ref_confidence'] = np.array([c.confidence for c in d.clusterCentroids])
            out['ref_index'] = np.array([c.index_freq * d.confidence.shape[1] + c.index_time
                                         for c in d.clusterCentroids])
            out['ref_sizes'] = np.array([c.sum() for c in d.clusters])
            out['steering'] = d.steeringVectorsFromCentroids()
    return d, out
