"""Generate tests/golden/sfnmf.npz by running the REFERENCE (the scratch
py2->py3 translation built by oracle/make_scratch_ref.py, as
tests/golden/make_golden_sf.py does):

    python tests/golden/make_golden_sfnmf.py

SFNMF_decomp_init (tools/nmf.py:161-360) at F = 65, N = 47, K = 13, Kf = 6,
Kr = 2, 4 iterations, the cases of tests/sfnmf_ref.py SFNMF_CASES: everything
drawn from the seeded global stream; the four inits supplied; each switch off
in turn; all four off (only the residual moves).  Per case `<case>_SX`, the
supplied `<case>_Winit` ..., `<case>_seed`, the six outputs `<case>_W` ...
`<case>_Hres` and `<case>_rand`, one np.random.rand() drawn after the call
(pins the draw order).

multiChanSourceF0Filter.initializeFreeMats (audioModel.py:2878-2908) on an
object built without its constructor (tests/sfnmf_ref.py bare_model: seeded
small dictionaries and Cx): the reference's own _initialize_structures(seed),
then initializeFreeMats(niter).  Recorded: `cls_Cx`, the dictionaries, the
state after the call (`cls_params_<j>`, `cls_<part>_<comp>_<factor>`) and
`cls_rand`.

Numbers only.  The scratch copy needs no patch beyond make_scratch_ref.py's.
"""
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
    import pyfasst.audioModel as am
    from pyfasst.tools.nmf import SFNMF_decomp_init
    import sfnmf_ref as S
    out = {}
    for name in sorted(S.SFNMF_CASES):
        seed = S.SFNMF_CASES[name][0]
        SX, inits = S.case_inputs(name)
        out[name + '_SX'] = SX
        out[name + '_seed'] = np.array(seed)
        for k, v in (inits or {}).items():
            out['%s_%s' % (name, k)] = v
        np.random.seed(seed)
        res = SFNMF_decomp_init(SX, verbose=0, **dict(S.case_kwargs(name), **(inits or {})))
        out[name + '_rand'] = np.array(np.random.rand())
        for n, v in zip(S.NAMES, res):
            assert np.all(np.isfinite(v)), (name, n)
            out['%s_%s' % (name, n)] = np.array(v)
    src, srcw, filt, Cx = S.class_dicts()
    c = S.CLASS_CFG
    out.update(cls_Cx=Cx, cls_src=np.array(src), cls_srcw=np.array(srcw), cls_filt=np.array(filt))
    m = S.bare_model(am.multiChanSourceF0Filter, src, srcw, filt, Cx)
    m._initialize_structures(seed=c['seed'])
    m.initializeFreeMats(niter=c['niter'])
    out['cls_rand'] = np.array(np.random.rand())
    assert m.spec_comps[0]['factor'][0]['FB'] is m.spec_comps[1]['factor'][0]['FB']
    for j, sc in m.spat_comps.items():
        out['cls_params_%d' % j] = np.array(sc['params'])
    for k, comp in m.spec_comps.items():
        for i, f in comp['factor'].items():
            for part in ('FB', 'FW', 'TW'):
                assert np.all(np.isfinite(f[part]))
                out['cls_%s_%d_%d' % (part, k, i)] = np.array(f[part])
    fn = os.path.join(HERE, "sfnmf.npz")
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
