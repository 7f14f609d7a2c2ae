"""Generate tests/golden/demix_<case>.npz by running the REFERENCE's own
demixTF.py (the scratch py2->py3 translation built by
oracle/make_scratch_ref.py, as tests/golden/make_golden_sigtools.py does):

    python tests/golden/make_golden_demix.py

The reference is Python 2 text that today's NumPy does not run.  After
make_scratch_ref.py's own list, the scratch copy of demixTF.py in /tmp is
patched with these mechanical substitutions (PATCHES below), and nothing else:

  * unary minus on boolean arrays -> `~`
    (:223 `-ind_cluster_theta_pts`, :300 `-ind_candidates`, :315 `-indicePeak`,
    :363-364 `-ind_cluster_pts`, :559 `- self.subTFpointSet`, :576 `- np.isnan`)
  * `/` on sizes and indices -> `//`
    (:304-305 `Nft*zoom/2`, :415 `(lengthData - oneMinLenData)/2`,
    :465 `self.neighbors / 2`, :1030-1031 `Nft * zoom / 2`)
  * `range(nbClusters)` followed by `.remove` -> `list(range(...))` and
    `self.sig_repr.values()` -> `list(...)` (both already made by 2to3)
  * `np.complex` (make_scratch_ref.py's list), `np.NaN` -> `np.nan`,
    `np.Inf` -> `np.inf`
  * integer slice bounds in getPeakCandidateIndices (:1060-1063):
    `infBounds[n]` / `supBounds[n]+1` -> `int(...)`

Numbers only: none of the reference's text is kept.  Recorded per case
(`tests/demix_ref.py` CASES, case_signal): `wav` (int16 [n, 2]), `fs`, the four
feature planes, per round `round_index` (flat centroid index), `round_theta`,
`round_phi`, `round_confidence`, `round_delta` (NaN allowed), `round_zoom`,
`round_size`, `round_remaining`, `clusters` (bit-packed, one row per round),
after refine_clusters() `ref_theta`, `ref_delta`, `ref_confidence`,
`ref_index`, `ref_sizes`, and `steering` (steeringVectorsFromCentroids()).
"""
import os
import re
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"

PATCHES = [
    (r"\*= \(-ind_cluster_theta_pts\)", "*= (~ind_cluster_theta_pts)"),
    (r"deltaDetFun\[-ind_candidates\]", "deltaDetFun[~ind_candidates]"),
    (r"deltaDetFun\[-indicePeak\]", "deltaDetFun[~indicePeak]"),
    (r"thetaVars\[-ind_cluster_pts\]", "thetaVars[~ind_cluster_pts]"),
    (r"y\[-ind_cluster_pts\]", "y[~ind_cluster_pts]"),
    (r"tmpConfidence\[\(- self\.subTFpointSet\)\]", "tmpConfidence[(~ self.subTFpointSet)]"),
    (r"ind_good_cluster = - np\.isnan\(", "ind_good_cluster = ~ np.isnan("),
    (r"stop=Nft\*zoom/2\)", "stop=Nft*zoom//2)"),
    (r"start=-Nft\*zoom/2,", "start=-Nft*zoom//2,"),
    (r"\(lengthData - oneMinLenData\)/2", "(lengthData - oneMinLenData)//2"),
    (r"start = self\.neighbors / 2", "start = self.neighbors // 2"),
    (r"\(Nft \* zoom / 2 - 1\)", "(Nft * zoom // 2 - 1)"),
    (r"deltaXiFFTmax = \(Nft \* zoom / 2\)", "deltaXiFFTmax = (Nft * zoom // 2)"),
    (r"np\.NaN\b", "np.nan"),
    (r"np\.Inf\b", "np.inf"),
    (r"indices_candidates\[infBounds\[n\]:\(supBounds\[n\]\+1\)\]",
     "indices_candidates[int(infBounds[n]):int(supBounds[n]+1)]"),
    (r"indices_candidates\[infBounds\[n\]:\]", "indices_candidates[int(infBounds[n]):]"),
    (r"indices_candidates\[:\(supBounds\[n\]\+1\)\]", "indices_candidates[:int(supBounds[n]+1)]"),
]


def patch_scratch():
    path = os.path.join(SCRATCH, "pyfasst", "demixTF.py")
    orig = path + ".orig"
    if not os.path.exists(orig):
        shutil.copy(path, orig)
    src = open(orig).read()
    for pat, rep in PATCHES:
        src, n = re.subn(pat, rep, src)
        if n == 0:
            raise RuntimeError("patch had no effect: " + pat)
    with open(path, "w") as fh:
        fh.write(src)


def main():
    import warnings
    warnings.simplefilter('ignore')
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import make_scratch_ref
    if not os.path.isdir(os.path.join(SCRATCH, "pyfasst")):
        make_scratch_ref.build(SCRATCH)
    patch_scratch()
    sys.path.insert(0, SCRATCH)
    import numpy as np
    import scipy.io.wavfile as wf
    if not hasattr(np, 'complex'):
        np.complex = complex
    import pyfasst.demixTF as dm
    import demix_ref as D

    for name in sorted(D.CASES):
        kw = dict(D.CASES[name])
        samples = D.case_signal(name)
        wavfn = "/tmp/%s.wav" % name
        wf.write(wavfn, D.FS, samples)
        d = dm.DEMIX(wavfn, verbose=0, **kw)
        zooms = []
        orig_cand = dm.TFPoint.getPeakCandidateIndices

        def cand(self, zoom=1, distBound=None, _o=orig_cand, _z=zooms):
            _z.append(zoom)
            return _o(self, zoom=zoom, distBound=distBound)
        dm.TFPoint.getPeakCandidateIndices = cand
        with np.errstate(all='ignore'):
            d.comp_clusters()
        dm.TFPoint.getPeakCandidateIndices = orig_cand
        L = d.confidence.shape[1]
        out = dict(wav=samples, fs=np.array(D.FS), confidence=d.confidence.copy(),
                   thetaAll=d.thetaAll.copy(), phiAll=d.phiAll.copy(),
                   thetaVarAll=d.thetaVarAll.copy())
        cc = d.clusterCentroids
        out['round_index'] = np.array([c.index_freq * L + c.index_time for c in cc])
        for k in ('theta', 'phi', 'confidence', 'delta'):
            out['round_' + k] = np.array([getattr(c, k) for c in cc], dtype=float)
        out['round_zoom'] = np.array(zooms)
        masks = np.array(d.clusters)
        out['round_size'] = masks.reshape(len(cc), -1).sum(axis=1)
        left = np.ones(masks.shape[1:], dtype=bool)
        rem = []
        for m in masks:
            left &= ~m
            rem.append(left.sum())
        out['round_remaining'] = np.array(rem)
        assert rem[-1] == d.subTFpointSet.sum()
        out['clusters'] = np.packbits(masks.reshape(len(cc), -1), axis=1)
        assert len(zooms) == len(cc)
        print(name, "rounds", len(cc), "NaN deltas", int(np.isnan(out['round_delta']).sum()),
              "zoom > 1 in", int((out['round_zoom'] > 1).sum()), "remaining", rem[-1])
        if name == 'demix_b':
            assert np.isnan(out['round_delta']).any(), "demix_b needs a centroid with no delta"
            assert (out['round_zoom'] > 1).any(), "demix_b needs a round with zoom > 1"
        with np.errstate(all='ignore'):
            d.refine_clusters()
        out['ref_theta'] = np.array([c.theta for c in d.clusterCentroids], dtype=float)
        out['ref_delta'] = np.array([c.delta for c in d.clusterCentroids], dtype=float)
        out['ref_confidence'] = np.array([c.confidence for c in d.clusterCentroids], dtype=float)
        out['ref_index'] = np.array([c.index_freq * L + c.index_time for c in d.clusterCentroids])
        out['ref_sizes'] = np.array([c.sum() for c in d.clusters])
        out['steering'] = d.steeringVectorsFromCentroids()
        print("   refined:", out['ref_theta'], out['ref_delta'], out['ref_confidence'],
              out['ref_sizes'])
        fn = os.path.join(HERE, name + ".npz")
        np.savez_compressed(fn, **out)
        print(fn, os.path.getsize(fn), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
