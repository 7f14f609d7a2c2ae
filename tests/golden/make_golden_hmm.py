"""Generate the discrete-state fixtures tests/golden/hmm_<case>.npz by running
the REFERENCE (the scratch py2->py3 translation built by
oracle/make_scratch_ref.py, as tests/golden/make_golden_spatial.py does):

    python tests/golden/make_golden_hmm.py            # all cases
    python tests/golden/make_golden_hmm.py hmm_gsmm

Each case runs in a fresh interpreter on make_golden.py's seeded `synth_wav`
signal plus the white noise make_golden_spatial.py adds: MultiChanHMM, 2
sources, K = 4, rank 1, wlen 128, hop 64, 4 iterations, 'conv' mixing, with

  hmm_shmm       makeItSHMM() (transitions 9 I + 1 row-normalised, fixed)
  hmm_shmm_free  TW_constr 'SHMM', TW_DP_frdm_prior 'free' (default transitions)
  hmm_gsmm       TW_constr 'GSMM', TW_DP_frdm_prior 'free' (default priors)

Recorded (numbers only): the WAV and its rate, the constructor arguments, the
per-iteration logliks, the final FB / FW / TW / TW_all / TW_DP_params of every
spectral component and the final mixing parameters, the decoded state
sequence of every component at every iteration `states` [iter, comp, T], and
`margin`.

The state sequence is a local of update_spectral_components, so it is read
off what the method leaves: TW has exactly one non-zero row per frame
(checked).  The margin is captured by wrapping numpy.argmin while that method
runs: over every argmin the reference takes, the smallest gap between the best
and second-best candidate relative to max(|best|, 1).  A case whose margin is
below MARGIN_MIN is refused: its decisions would rest on rounding.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"
NOISE_STD = 1000.0
MARGIN_MIN = 1e-6

CFG = dict(nbComps=2, nbNMFComps=4, spatial_rank=1, n=4000, fs=8000,
           kw=dict(iter_num=4, wlen=128, hopsize=64))
CASES = ("hmm_shmm", "hmm_shmm_free", "hmm_gsmm")


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
    from tw_constr_ref import HMM_CASES, argmin_margin
    cfg = CFG
    seed = sum(map(ord, name)) % 1000
    data = synth_wav(cfg['n'], cfg['fs'], seed).astype(np.float64)
    data += NOISE_STD * np.random.RandomState(seed + 1).randn(*data.shape)
    data = np.clip(data, -32768, 32767).astype(np.int16)
    wav = "/tmp/golden_%s.wav" % name
    wf.write(wav, cfg['fs'], data)
    np.random.seed(0)
    m = am.MultiChanHMM(wav, nbComps=cfg['nbComps'], nbNMFComps=cfg['nbNMFComps'],
                        spatial_rank=cfg['spatial_rank'], verbose=0, **cfg['kw'])
    m.makeItConvolutive()
    HMM_CASES[name](m)
    keys = sorted(m.spec_comps.keys())
    states, margin = [], [np.inf]
    orig_update = m.update_spectral_components
    orig_argmin = np.argmin

    def argmin(x, axis=None, *a, **kw):
        margin[0] = min(margin[0], argmin_margin(x, axis))
        return orig_argmin(x, axis, *a, **kw)

    def update(hat_W):
        np.argmin = argmin
        try:
            out = orig_update(hat_W)
        finally:
            np.argmin = orig_argmin
        seqs = []
        for k in keys:
            TW = m.spec_comps[k]['factor'][0]['TW']
            assert np.all(np.sum(TW != 0, axis=0) == 1), "one non-zero TW row per frame"
            seqs.append(np.argmax(TW != 0, axis=0).astype(np.int32))
        states.append(seqs)
        return out
    m.update_spectral_components = update
    logliks = m.estim_param_a_post_model()
    if not margin[0] >= MARGIN_MIN:
        raise SystemExit("%s: decision margin %.3g < %g: case refused" % (name, margin[0],
                                                                         MARGIN_MIN))
    ctor = dict(nbComps=cfg['nbComps'], nbNMFComps=cfg['nbNMFComps'],
                spatial_rank=cfg['spatial_rank'], kw=cfg['kw'])
    out = {'wav': data, 'fs': np.array(cfg['fs']), 'ctor': np.array(json.dumps(ctor)),
           'logliks': np.array(logliks), 'states': np.array(states),
           'margin': np.array(margin[0])}
    for j in range(len(m.spat_comps)):
        out['final_params_%d' % j] = np.array(m.spat_comps[j]['params'])
    for k in keys:
        fac = m.spec_comps[k]['factor'][0]
        for part in ('FB', 'FW', 'TW', 'TW_all', 'TW_DP_params'):
            out['final_%s_%d' % (part, k)] = np.array(fac[part])
    fn = os.path.join(HERE, name + ".npz")
    np.savez_compressed(fn, **out)
    print(name, "margin %.3g" % margin[0], "logliks", logliks, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        run_case(sys.argv[2])
        sys.exit(0)
    import make_scratch_ref
    if not os.path.isdir(os.path.join(SCRATCH, "pyfasst")):
        make_scratch_ref.build(SCRATCH)
    for name in sys.argv[1:] or list(CASES):
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", name])
