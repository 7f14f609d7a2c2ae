"""Generate the spatial-filter fixtures tests/golden/spatial_<case>*.npz by
running the REFERENCE (the scratch py2->py3 translation built by
oracle/make_scratch_ref.py, as tests/golden/make_golden.py does):

    python tests/golden/make_golden_spatial.py            # all cases
    python tests/golden/make_golden_spatial.py spatial_conv

Each case runs in a fresh interpreter, as in make_golden.py, on that file's
seeded `synth_wav` signal plus independent white noise in each channel
(NOISE_STD, about 5 % of the peak).  Without the noise no seed passes the
conditioning guard below: synth_wav's second source is a 5-tap moving
average, whose spectral zeros (fs/5 and 2 fs/5, bins 51 and 102 of 256) leave
one source in those bins, so the free 'conv' update makes every mixing vector
collinear there (measured: cond(R_aa) = 8.6e5 for spatial_conv, 1.8e6 for
spatial_conv_j1, 4.5e4 for spatial_mqt; with the noise 18, 194 and 26).
Recorded per case: the WAV and its rate, the
constructor arguments, the 'conv' mixing parameters after the EM iterations,
and what separate_spatial_filter_comp (audioModel.py:891-1061) and
gcc_phat_tdoa_2d (:1316-1324) make of them:

  WG        [J, 2, 2, F]  the arrays compute_Wiener_gain_2d returned, which the
                          method then divides in place by their real trace
  images_n  [2, F, T]     tft.transfo at each tft.invertTransform call
  sep_wav_n               the WAV files it wrote (names in `files`)
  gcc       [fsize, T]    gcc_phat_tdoa_2d()
  cond_max                max over the bins of cond(R_aa(f)); a case above
                          COND_MAX is refused (the tests' gain tolerance
                          follows from this bound)

Only numbers are stored.  A case's arrays go into spatial_<case>.npz and, when
that would pass PART_BYTES, into further spatial_<case>.part<k>.npz files
(tests/spatial_filter_ref.py load_fixture merges them).
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"
COND_MAX = 1e3
NOISE_STD = 1000.0
PART_BYTES = 900 * 1024

CASES = {
    "spatial_conv": dict(nbComps=3, nbNMFComps=8, spatial_rank=2, n=6000, fs=8000,
                         kw=dict(iter_num=2, wlen=256, hopsize=64)),
    "spatial_conv_j1": dict(nbComps=1, nbNMFComps=3, spatial_rank=[2], n=3000, fs=8000,
                            kw=dict(iter_num=2, wlen=128, hopsize=32)),
    # the em_mqt structure of make_golden.py: the image path + the host inverse
    "spatial_mqt": dict(nbComps=2, nbNMFComps=6, spatial_rank=2, n=4000, fs=8000,
                        kw=dict(iter_num=2, wlen=256, hopsize=64, transf='mqt', tffmin=200,
                                tfbpo=12)),
}


def save_parts(name, out):
    """Greedy split of the arrays over files of at most PART_BYTES (raw)."""
    import glob
    import numpy as np
    for old in glob.glob(os.path.join(HERE, name + ".npz")) + \
            glob.glob(os.path.join(HERE, name + ".part*.npz")):
        os.remove(old)
    parts, size = [{}], 0
    for k, v in out.items():
        nb = np.asarray(v).nbytes
        if parts[-1] and size + nb > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += nb
    for i, p in enumerate(parts):
        fn = name + (".npz" if i == 0 else ".part%d.npz" % i)
        np.savez_compressed(os.path.join(HERE, fn), **p)
        print(fn, os.path.getsize(os.path.join(HERE, fn)), sorted(p))


def run_case(name):
    import warnings
    warnings.simplefilter('ignore')
    sys.path.insert(0, SCRATCH)
    sys.path.insert(0, HERE)
    import numpy as np
    import scipy.io.wavfile as wf
    import pyfasst.audioModel as am
    from make_golden import synth_wav
    cfg = CASES[name]
    seed = sum(map(ord, name)) % 1000
    data = synth_wav(cfg['n'], cfg['fs'], seed).astype(np.float64)
    data += NOISE_STD * np.random.RandomState(seed + 1).randn(*data.shape)
    data = np.clip(data, -32768, 32767).astype(np.int16)
    wav = "/tmp/golden_%s.wav" % name
    wf.write(wav, cfg['fs'], data)
    np.random.seed(0)
    m = am.MultiChanNMFConv(wav, nbComps=cfg['nbComps'], nbNMFComps=cfg['nbNMFComps'],
                            spatial_rank=cfg['spatial_rank'], verbose=0, **cfg['kw'])
    m.makeItConvolutive()
    m.estim_param_a_post_model()     # the params now differ from bin to bin
    J = len(m.spat_comps)
    ctor = dict(nbComps=cfg['nbComps'], nbNMFComps=cfg['nbNMFComps'],
                spatial_rank=cfg['spatial_rank'], kw=cfg['kw'])
    out = {'wav': data, 'fs': np.array(cfg['fs']), 'ctor': np.array(json.dumps(ctor))}
    for j in range(J):
        assert m.spat_comps[j]['mix_type'] == 'conv'
        out['params_%d' % j] = np.array(m.spat_comps[j]['params'])
    # conditioning of R_aa(f) = mean_n sum_r a_r a_r^H
    P = [out['params_%d' % j] for j in range(J)]
    Raa = sum(np.einsum('rcf,rdf->fcd', p, np.conj(p)) for p in P) / J
    cond = float(np.max(np.linalg.cond(Raa)))
    if not cond <= COND_MAX:
        raise SystemExit("%s: max cond(R_aa) = %.3g > %g: case refused" % (name, cond, COND_MAX))
    out['cond_max'] = np.array(cond)
    gains, images = [], []
    orig_wg = m.compute_Wiener_gain_2d

    def wg(*a, **kw):
        g = orig_wg(*a, **kw)
        gains.append(g)          # the caller's in-place trace division lands here
        return g
    m.compute_Wiener_gain_2d = wg
    orig_inv = m.tft.invertTransform

    def capture():
        images.append(np.array(m.tft.transfo))
        return orig_inv()
    m.tft.invertTransform = capture
    outdir = "/tmp/golden_%s_sep" % name
    os.makedirs(outdir, exist_ok=True)
    m.separate_spatial_filter_comp(dir_results=outdir)
    m.tft.invertTransform = orig_inv
    assert len(gains) == J and len(images) == 2 * J
    out['WG'] = np.array(gains)
    out['files'] = np.array([os.path.basename(f) for f in m.files['spatial']])
    for n, fn in enumerate(m.files['spatial']):
        out['sep_wav_%d' % n] = wf.read(fn)[1]
    out['gcc'] = np.array(m.gcc_phat_tdoa_2d())
    for n in range(J):
        out['images_%d' % n] = np.array(images[2 * n:2 * n + 2])
    print(name, "cond_max %.3g" % cond, {k: np.shape(v) for k, v in out.items()
                                        if k in ('WG', 'images_0', 'gcc', 'sep_wav_0')})
    save_parts(name, out)


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
