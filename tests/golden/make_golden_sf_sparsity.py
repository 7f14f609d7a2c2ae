"""Generate tests/golden/sf_sparse.npz by running the REFERENCE's sparsity
schedule (the scratch py2->py3 translation built by oracle/make_scratch_ref.py,
as tests/golden/make_golden_sf.py does):

    python tests/golden/make_golden_sf_sparsity.py

The model is make_golden_sf.py's `sf_inst` (F = 65, 3 components: two
source / filter components of tests/sf_ref.py's two_factor spec and a
single-factor one at K = 4) with m.nbComps = 3 and spec_comps[j]['sparsity'] =
[3, False, 2][j] (tests/sf_sparsity_ref.py SPARSE_LENGTHS): the third,
single-factor component is reweighed too.  The model is a
MultiChanNMFInst_FASST, so the two methods of multiChanSourceF0Filter under
test are called as plain functions on it:

  * reweigh_sparsity_constraint(m, sigma) once at sigma = 169 and once at
    sigma = 9 on copies of the initial parameters (`rw169_TW_<comp>`,
    `rw9_TW_<comp>`: factor 0's TW of every component);
  * estim_param_a_post_model(m), 4 iterations (`logliks`, `final_*`).

Recorded (numbers only): what make_golden_sf.py records for the initial and
final state, the sparsity lengths, and the two reweighed TW sets.
"""
import copy
import json
import os
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"
NAME = "sf_sparse"


def run_case():
    import warnings
    warnings.simplefilter('ignore')
    sys.path.insert(0, SCRATCH)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import scipy.io.wavfile as wf
    import pyfasst.audioModel as am
    from make_golden import synth_wav
    from make_golden_sf import NOISE_STD
    from sf_ref import PARTS, SF_CFG, SF_FIXTURES, two_factor
    from sf_sparsity_ref import SPARSE_CASE, SPARSE_LENGTHS
    cfg = SF_FIXTURES[SPARSE_CASE]
    seed = sum(map(ord, SPARSE_CASE)) % 1000
    data = synth_wav(SF_CFG['n'], SF_CFG['fs'], seed).astype(np.float64)
    data += NOISE_STD * np.random.RandomState(seed + 1).randn(*data.shape)
    data = np.clip(data, -32768, 32767).astype(np.int16)
    wav = "/tmp/golden_%s.wav" % NAME
    wf.write(wav, SF_CFG['fs'], data)
    np.random.seed(0)
    m = am.MultiChanNMFInst_FASST(wav, nbComps=SF_CFG['nbComps'], nbNMFComps=SF_CFG['nbNMFComps'],
                                  spatial_rank=cfg['spatial_rank'], verbose=0, **cfg['kw'])
    two_factor(m, cfg['spec'])
    m.nbComps = SF_CFG['nbComps']
    for j, L in enumerate(SPARSE_LENGTHS):
        m.spec_comps[j]['sparsity'] = L
    cls = am.multiChanSourceF0Filter
    m.reweigh_sparsity_constraint = types.MethodType(cls.reweigh_sparsity_constraint, m)
    ctor = dict(nbComps=SF_CFG['nbComps'], nbNMFComps=SF_CFG['nbNMFComps'],
                spatial_rank=cfg['spatial_rank'], kw=cfg['kw'])
    out = {'wav': data, 'fs': np.array(SF_CFG['fs']), 'ctor': np.array(json.dumps(ctor)),
           'psd_lim0': np.asarray(m.noise['ann_PSD_lim'][0]),
           'psd_lim1': np.asarray(m.noise['ann_PSD_lim'][1]),
           'sparsity': np.array([int(L) for L in SPARSE_LENGTHS])}

    def dump(prefix):
        for j, sc in m.spat_comps.items():
            out['%sparams_%d' % (prefix, j)] = np.array(sc['params'])
        for k, comp in m.spec_comps.items():
            for i, f in comp['factor'].items():
                for part in PARTS:
                    out['%s%s_%d_%d' % (prefix, part, k, i)] = np.array(f[part])
                out['priors_%d_%d' % (k, i)] = np.array([f[p + '_frdm_prior'] for p in PARTS])
    dump('init_')
    init = copy.deepcopy(m.spec_comps)
    for sigma in (169., 9.):
        m.spec_comps = copy.deepcopy(init)
        cls.reweigh_sparsity_constraint(m, sigma)
        for k, comp in m.spec_comps.items():
            out['rw%d_TW_%d' % (sigma, k)] = np.array(comp['factor'][0]['TW'])
    m.spec_comps = copy.deepcopy(init)
    logliks = cls.estim_param_a_post_model(m)
    out['logliks'] = np.real(logliks)
    out['final_psd'] = np.asarray(m.noise['PSD'])
    dump('final_')
    fn = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(fn, **out)
    print(NAME, "logliks", logliks, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        run_case()
        sys.exit(0)
    import make_scratch_ref
    if not os.path.isdir(os.path.join(SCRATCH, "pyfasst")):
        make_scratch_ref.build(SCRATCH)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case"])
