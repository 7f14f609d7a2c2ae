"""Generate the two-factor fixtures tests/golden/sf_<case>.npz by running the
REFERENCE (the scratch py2->py3 translation built by
oracle/make_scratch_ref.py, as tests/golden/make_golden_hmm.py does):

    python tests/golden/make_golden_sf.py            # all cases
    python tests/golden/make_golden_sf.py sf_inst

Each case runs in a fresh interpreter on make_golden.py's seeded `synth_wav`
signal plus white noise: a MultiChanNMFInst_FASST (MultiChanNMFConv and
makeItConvolutive() for the 'conv' case), wlen 128, hop 64, 3 sources, whose
first two spectral components are replaced by hand with two-factor components
(tests/sf_ref.py: SF_FIXTURES and two_factor, seeded positive random
matrices); the third stays single-factor (K = 4) and free.  4 iterations.

  sf_inst  'inst' rank 1; factor 0: FB 65 x 13 fixed, FW = I fixed, TW free;
           factor 1: FB 65 x 6 fixed, FW 6 x 3 free, TW 3 x T free; omega 1
  sf_conv  'conv' rank 2; factor 0: FB free; factor 1: TW fixed; omega 0.7

Recorded (numbers only): the WAV and its rate, the constructor arguments, the
annealing limits, every initial and final matrix (`init_/final_<part>_<comp>_
<factor>`, `priors_<comp>_<factor>`), the initial and final mixing parameters,
the logliks, and |S| of the separated images (`absS`).

The scratch copy needs no patch beyond make_scratch_ref.py's for these cases.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"
NOISE_STD = 1000.0


def run_case(name):
    import warnings
    warnings.simplefilter('ignore')
    sys.path.insert(0, SCRATCH)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import scipy.io.wavfile as wf
    import pyfasst.audioModel as am
    from make_golden import synth_wav
    from sf_ref import PARTS, SF_CFG, SF_FIXTURES, two_factor
    cfg = SF_FIXTURES[name]
    seed = sum(map(ord, name)) % 1000
    data = synth_wav(SF_CFG['n'], SF_CFG['fs'], seed).astype(np.float64)
    data += NOISE_STD * np.random.RandomState(seed + 1).randn(*data.shape)
    data = np.clip(data, -32768, 32767).astype(np.int16)
    wav = "/tmp/golden_%s.wav" % name
    wf.write(wav, SF_CFG['fs'], data)
    np.random.seed(0)
    cls = am.MultiChanNMFConv if cfg['conv'] else am.MultiChanNMFInst_FASST
    m = cls(wav, nbComps=SF_CFG['nbComps'], nbNMFComps=SF_CFG['nbNMFComps'],
            spatial_rank=cfg['spatial_rank'], verbose=0, **cfg['kw'])
    if cfg['conv']:
        m.makeItConvolutive()
    two_factor(m, cfg['spec'])
    ctor = dict(nbComps=SF_CFG['nbComps'], nbNMFComps=SF_CFG['nbNMFComps'],
                spatial_rank=cfg['spatial_rank'], kw=cfg['kw'])
    out = {'wav': data, 'fs': np.array(SF_CFG['fs']), 'ctor': np.array(json.dumps(ctor)),
           'psd_lim0': np.asarray(m.noise['ann_PSD_lim'][0]),
           'psd_lim1': np.asarray(m.noise['ann_PSD_lim'][1])}

    def dump(prefix):
        for j, sc in m.spat_comps.items():
            out['%sparams_%d' % (prefix, j)] = np.array(sc['params'])
        for k, comp in m.spec_comps.items():
            for i, f in comp['factor'].items():
                for part in PARTS:
                    out['%s%s_%d_%d' % (prefix, part, k, i)] = np.array(f[part])
                out['priors_%d_%d' % (k, i)] = np.array([f[p + '_frdm_prior'] for p in PARTS])
    dump('init_')
    logliks = m.estim_param_a_post_model()
    out['logliks'] = np.real(logliks)
    out['final_psd'] = np.asarray(m.noise['PSD'])
    dump('final_')
    images = []
    orig = m.tft.invertTransform

    def capture():
        images.append(np.array(m.tft.transfo))
        return orig()
    m.tft.invertTransform = capture
    outdir = "/tmp/golden_%s_sep" % name
    os.makedirs(outdir, exist_ok=True)
    m.separate_spat_comps(dir_results=outdir)
    J = len(m.spat_comps)
    out['absS'] = np.abs(np.array(images).reshape(J, 2, *images[0].shape))
    fn = os.path.join(HERE, name + ".npz")
    np.savez_compressed(fn, **out)
    print(name, "logliks", logliks, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        run_case(sys.argv[2])
        sys.exit(0)
    import make_scratch_ref
    from sf_ref import SF_FIXTURES
    if not os.path.isdir(os.path.join(SCRATCH, "pyfasst")):
        make_scratch_ref.build(SCRATCH)
    for name in sys.argv[1:] or sorted(SF_FIXTURES):
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", name])
