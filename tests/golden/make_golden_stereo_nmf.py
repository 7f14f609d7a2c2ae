"""Generate tests/golden/stereo_nmf.npz by running the REFERENCE's own
stereo_NMF (SeparateLeadStereo/SIMM/SIMM.py:945-1104) through the scratch
py2->py3 translation built by oracle/make_scratch_ref.py:

    python tests/golden/make_golden_stereo_nmf.py

Cases (tests/stereo_nmf_ref.py CASES): `rand` (nothing supplied), `given`
(WM0 and HM0 supplied), `omega07` (updateRulePower = 0.7), `wrongshape` (a WM0
with one row too many, replaced by the draw), `r1` (R = 1).  Per case the data
`<case>_SXR`, `<case>_SXL`, the supplied `<case>_WM0` / `<case>_HM0`,
`<case>_seed`, the four outputs `<case>_betaR` ... `<case>_WM` and
`<case>_rand`, one np.random.rand() drawn after the call (pins the position
the global stream is left at).

Numbers only.  The scratch copy needs no patch beyond make_scratch_ref.py's.
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"


def main():
    import warnings
    warnings.simplefilter('ignore')
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import make_scratch_ref
    if not os.path.isdir(os.path.join(SCRATCH, "pyfasst")):
        make_scratch_ref.build(SCRATCH)
    sys.path.insert(0, SCRATCH)
    import numpy as np
    from pyfasst.SeparateLeadStereo.SIMM.SIMM import stereo_NMF
    import stereo_nmf_ref as S
    out = {}
    for name in sorted(S.CASES):
        SXR, SXL, kw, seed = S.case_inputs(name)
        out[name + '_SXR'] = SXR
        out[name + '_SXL'] = SXL
        out[name + '_seed'] = np.array(seed)
        for k in ('WM0', 'HM0'):
            if k in kw:
                out['%s_%s' % (name, k)] = kw[k]
        np.random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):     # the wrong-shape message
            res = stereo_NMF(SXR, SXL, verbose=False, displayEvolution=False, **kw)
        out[name + '_rand'] = np.array(np.random.rand())
        for n, v in zip(S.NAMES, res):
            assert np.all(np.isfinite(v)), (name, n)
            out['%s_%s' % (name, n)] = np.array(v)
    fn = os.path.join(HERE, "stereo_nmf.npz")
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
