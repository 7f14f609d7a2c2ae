"""Generate tests/golden/sigtools.npz by running the REFERENCE's own
tools/signalTools.py (the scratch py2->py3 translation built by
oracle/make_scratch_ref.py, as tests/golden/make_golden_sfnmf.py does):

    python tests/golden/make_golden_sigtools.py

The cases are those of tests/sigtools_ref.py: prinComp2D (`pca_<case>_X0`,
`_X1`, `_nb` in; `_lambdaM`, `_lambdam`, `_vM`, `_vm` out), medianFilter
(`med_<case>_in`, `_length`, `_out`), f0detectionFunction (`hs_<case>_TF` in;
`_hs`, `_f0` out), sortSpectrum (`sort_in`; `sort_sorted`, `sort_f0s`,
`sort_hs`, `sort_hp`, `sort_f0table`, `sort_order`) and invHermMat2D
(`inv_<case>_a00` ... in; `_i00`, `_i01`, `_i11` out).

Numbers only.  The reference text is not patched beyond make_scratch_ref.py's
list.  Two things are set in THIS process before the import, for the NumPy the
reference was written against: the np.complex alias, if the installed NumPy
lacks it, and, in the module's own `np` name, a zeros() that truncates a float
dimension as that NumPy did (np.zeros([F0number, nframes]), :238, with
F0number = np.ceil(...)).  The reference's "No freq bins" prints are dropped.
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"


class _OldNumpy(object):
    """The numpy module with the zeros() of the reference's time."""

    def __init__(self, np):
        self._np = np

    def __getattr__(self, name):
        return getattr(self._np, name)

    def zeros(self, shape, *args, **kwargs):
        if isinstance(shape, (list, tuple)):
            shape = [int(s) for s in shape]
        return self._np.zeros(shape, *args, **kwargs)


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
    if not hasattr(np, 'complex'):
        np.complex = complex
    import pyfasst.tools.signalTools as st
    import sigtools_ref as S
    st.np = _OldNumpy(np)
    out = {}
    for name in sorted(S.PCA_CASES):
        X0, X1, nb = S.pca_inputs(name)
        res = st.prinComp2D(X0, X1, neighborNb=nb)
        out.update({'pca_%s_X0' % name: X0, 'pca_%s_X1' % name: X1, 'pca_%s_nb' % name: np.array(nb)})
        for k, v in zip(('lambdaM', 'lambdam', 'vM', 'vm'), res):
            assert not np.any(np.isnan(v)), (name, k)
            out['pca_%s_%s' % (name, k)] = v
    for name in sorted(S.MEDIAN_CASES):
        x, length = S.median_input(name)
        out.update({'med_%s_in' % name: x, 'med_%s_length' % name: np.array(length),
                    'med_%s_out' % name: st.medianFilter(x, length=length)})
    sink = io.StringIO()
    for name in sorted(S.HS_CASES):
        TF, kw = S.hs_input(name)
        with contextlib.redirect_stdout(sink):
            hs, f0 = st.f0detectionFunction(TF, **kw)
        assert np.all(np.isfinite(hs)) and np.any(hs > 0), name
        out.update({'hs_%s_TF' % name: TF, 'hs_%s_hs' % name: hs, 'hs_%s_f0' % name: f0})
    spec = S.sort_input()
    with contextlib.redirect_stdout(sink):
        res = st.sortSpectrum(spec, numberHarmonicsHS=S.SORT_HS, numberHarmonicsHP=S.SORT_HP,
                              **S.SORT_KW)
    sal = np.sort(res[2] * res[3], axis=0)
    assert np.all(sal[-1] > sal[-2] * (1 + 1e-6)), "salience maxima are not distinct"
    assert np.unique(res[1]).size == res[1].size
    out['sort_in'] = spec
    for k, v in zip(('sorted', 'f0s', 'hs', 'hp', 'f0table'), res):
        out['sort_' + k] = v
    out['sort_order'] = np.argsort(res[4][np.argmax(res[2] * res[3], axis=0)])
    for name, (a00, a01, a11) in sorted(S.inv_inputs().items()):
        res = st.invHermMat2D(a00, a01, a11)
        for k, v in zip(('a00', 'a01', 'a11', 'i00', 'i01', 'i11'), (a00, a01, a11) + tuple(res)):
            out['inv_%s_%s' % (name, k)] = np.array(v)
    fn = os.path.join(HERE, "sigtools.npz")
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
