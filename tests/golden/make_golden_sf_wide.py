"""Generate tests/golden/sf_wide.npz by running the REFERENCE class
multiChanSourceF0Filter (the scratch py2->py3 translation built by
oracle/make_scratch_ref.py, as tests/golden/make_golden_sf.py does) at a small
shape whose F0 dictionary is wider than 128 columns:

    python tests/golden/make_golden_sf_wide.py

make_golden.py's seeded `synth_wav` signal plus white noise, 5000 samples at
8 kHz; wlen 256, hop 64 (F = 129); minF0 100, maxF0 800, stepnoteF0 4: 3
octaves x 48 + 1 F0s and the ones column, 146 columns (asserted > 128 and no
multiple of 16); nbComps 3 (two source / filter components sharing ONE
dictionary and ONE weight matrix, one residual NMF component), 6 Hann filter
bumps, 3 filter weights; 3 iterations.

Recorded (numbers only): the WAV and its rate, the constructor arguments, the
annealing limits, the initial state (the class's own, drawn with a seed, after
its renormalisation, which already turns the identity weights into a diagonal
matrix; then brought to the level of the clip, see main()), the final state,
the logliks and |S| of the separated images (every 4th frame).  An
array held by several factors (the F0 dictionary, its weights and the filter
basis are each ONE array in both source / filter components) is stored once:
`alias_<part>_<k>_<i>` names the first factor "<k>_<i>" holding it.

Beyond make_scratch_ref.py's patches the scratch copy needs patch_scratch()'s.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"
NOISE_STD = 1000.0
PARTS = ('FB', 'FW', 'TW')
CFG = dict(n=5000, fs=8000, seed=11,
           ctor=dict(nbComps=3, nbNMFResComps=2, nbFilterComps=6, nbFilterWeigs=[3], minF0=100,
                     maxF0=800, stepnoteF0=4, spatial_rank=1, iter_num=3, wlen=256, hopsize=64))


def patch_scratch():
    """The class constructor reaches one file make_scratch_ref.py's list does
    not cover: float sizes and slice bounds in the Hann filter basis, the same
    mechanical fix as its separateLeadFunctions.py entries (idempotent)."""
    import re
    path = os.path.join(SCRATCH, "pyfasst", "sourcefilter", "filter.py")
    with open(path) as fh:
        src = fh.read()
    for pat, rep in ((r"np\.hanning\(lengthSineWindow\)", "np.hanning(int(lengthSineWindow))"),
                     (r"np\.zeros\(\[sizeBigWindow \* 2, 1\]\)", "np.zeros([int(sizeBigWindow * 2), 1])"),
                     (r"\[\(sizeBigWindow - lengthSineWindow / 2\.0\):\\\n\s+\(sizeBigWindow \+ "
                      r"lengthSineWindow / 2\.0\)\]",
                      "[int(sizeBigWindow - lengthSineWindow / 2.0):"
                      "int(sizeBigWindow + lengthSineWindow / 2.0)]")):
        src = re.sub(pat, rep, src)
    with open(path, "w") as fh:
        fh.write(src)


def main():
    import warnings
    warnings.simplefilter('ignore')
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import make_scratch_ref
    if not os.path.isdir(os.path.join(SCRATCH, "pyfasst")):
        make_scratch_ref.build(SCRATCH)
    patch_scratch()
    sys.path.insert(0, SCRATCH)
    sys.path.insert(0, HERE)
    import numpy as np
    import scipy.io.wavfile as wf
    import pyfasst.audioModel as am
    from make_golden import synth_wav
    data = synth_wav(CFG['n'], CFG['fs'], CFG['seed']).astype(np.float64)
    data += NOISE_STD * np.random.RandomState(CFG['seed'] + 1).randn(*data.shape)
    data = np.clip(data, -32768, 32767).astype(np.int16)
    wav = "/tmp/golden_sf_wide.wav"
    wf.write(wav, CFG['fs'], data)
    import tempfile
    # the reference caches its F0 dictionary in the working directory, and
    # loads whatever file of that name it finds there: start from an empty one
    os.chdir(tempfile.mkdtemp())
    np.random.seed(0)
    m = am.multiChanSourceF0Filter(wav, verbose=0, **CFG['ctor'])
    # (the constructor seeds its draws from the clock: draw the state again, seeded)
    m._initialize_structures(seed=CFG['seed'])
    Kb = m.spec_comps[0]['factor'][0]['FB'].shape[1]
    assert Kb > 128 and Kb % 16, Kb
    # The constructor's initial state is not scaled to the signal: at this F0
    # grid the source / filter components start with powers up to 1e11 against
    # a clip of mean power 2 and a noise floor of 0.03, and the reference's
    # posterior covariance (Sigma_s - G A Sigma_s) then cancels to rounding
    # noise: a 1e-15 relative change of TW moved its own final parameters by
    # 2.6e+1 relative.  No implementation can be held to such a run.  The
    # activations of each component's last factor (where the renormalisation
    # leaves the component's energy) are scaled so that the component's mean
    # power is the clip's mean channel power shared over the components; the
    # estimation below is the reference's own, from that state.
    level = 0.5 * np.mean(np.real(m.Cx[0]) + np.real(m.Cx[2])) / len(m.spat_comps)
    for j in range(len(m.spat_comps) - 1):
        facs = m.spec_comps[j]['factor']
        facs[max(facs)]['TW'] *= level / np.mean(m.comp_spat_comp_power(j))
    out = {'wav': data, 'fs': np.array(CFG['fs']), 'ctor': np.array(json.dumps(CFG['ctor'])),
           'psd_lim0': np.asarray(m.noise['ann_PSD_lim'][0]),
           'psd_lim1': np.asarray(m.noise['ann_PSD_lim'][1])}
    first = {}   # (part, id of the array) -> the first "<k>_<i>" holding it

    def dump(prefix):
        for j, sc in m.spat_comps.items():
            out['%sparams_%d' % (prefix, j)] = np.array(sc['params'])
        for k, comp in m.spec_comps.items():
            for i, f in comp['factor'].items():
                for part in PARTS:
                    here = '%d_%d' % (k, i)
                    held = first.setdefault((prefix, part, id(f[part])), here)
                    out['alias_%s_%s' % (part, here)] = np.array(held)
                    if held == here:
                        out['%s%s_%s' % (prefix, part, here)] = np.array(f[part])
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
    outdir = "/tmp/golden_sf_wide_sep"
    os.makedirs(outdir, exist_ok=True)
    m.separate_spat_comps(dir_results=outdir)
    J = len(m.spat_comps)
    # every 4th frame of the images: the whole of |S| would not fit the fixture
    out['absS_step'] = np.array(4)
    out['absS'] = np.abs(np.array(images).reshape(J, 2, *images[0].shape))[..., ::4]
    fn = os.path.join(HERE, "sf_wide.npz")
    np.savez_compressed(fn, **out)
    print("Kb", Kb, "T", m.nbFramesSigRepr, "logliks", logliks, os.path.getsize(fn), "bytes")
    assert os.path.getsize(fn) < 1 << 20


if __name__ == "__main__":
    main()
