"""Generate tests/golden/cqt_cells.npz by running the REFERENCE's own
tftransforms/minqt.py with perfRast=0 (the scratch py2->py3 translation built
by oracle/make_scratch_ref.py, as the other generators do):

    python tests/golden/make_golden_cqt_cells.py

The non-raster branch has float sizes and indices that make_scratch_ref.py's
patch list does not reach.  They are cast to int in THIS generator's own
scratch copy (EXTRA below), and nothing else of the reference is changed:

  computeCQT (:509-516)     `for n in np.arange(nframes)` of the cell loop,
                            framestart / framestop built from cqtkernel.fftHOP,
                            n=cqtkernel.FFTLen
  cellCQT2spCQT (:875-880)  the two dimensions of the np.zeros of _spCQT
  cellCQT2spCQT (:947)      the final [:, :spCQTframes]

Cases and signals are those of tests/cqt_cells_ref.py (CASES, signal, modify).
Per case <c>: `<c>_x`, `<c>_scalars` (atomHOP, first_center, winNr, fftHOP,
FFTLen, octaveNr), `<c>_nframes`, `<c>_cell<i>` (and `<c>_cell_linear`),
`<c>_sp` (the transfo getter), `<c>_y` (invertTransform), `<c>_tstamps`,
`<c>_fstamps`; for the round-trip cases, after modify(<c>_sp) is assigned
to transfo, also `<c>_rt_cell<i>` and `<c>_rt_y`.  `<c>_del`
records what the reference does on `del transfo` followed by the getter
(1: AttributeError).  Numbers only.
"""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch_cells"

EXTRA = [
    # 16 / 20 spaces: computeCQT's loop, not HybridCQTransfo's copy of it
    (r"(?m)^ {16}for n in np\.arange\(nframes\):\n( +)if self\.verbose>1:",
     r"                for n in np.arange(int(nframes)):\n\1if self.verbose>1:"),
    (r"(?m)^ {20}framestart = n\*cqtkernel\.fftHOP\n",
     "                    framestart = int(n*cqtkernel.fftHOP)\n"),
    (r"(?m)^ {20}framestop = framestart \+ cqtkernel\.FFTLen\n",
     "                    framestop = int(framestart + cqtkernel.FFTLen)\n"),
    (r"X = np\.fft\.fft\(x\[framestart:framestop\],\n\s+n=cqtkernel\.FFTLen\)",
     "X = np.fft.fft(x[framestart:framestop], n=int(cqtkernel.FFTLen))"),
    (r"self\._spCQT = np\.zeros\(\[self\.cqtkernel\.bins \* \n\s+self\.octaveNr,\n"
     r"\s+self\.cellCQT\[0\]\.shape\[1\] \*\n\s+self\.cqtkernel\.winNr\],",
     "self._spCQT = np.zeros([int(self.cqtkernel.bins * self.octaveNr), "
     "int(self.cellCQT[0].shape[1] * self.cqtkernel.winNr)],"),
    (r"self\._spCQT\[:,:spCQTframes\]", "self._spCQT[:,:int(spCQTframes)]"),
]


def scratch():
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import make_scratch_ref
    make_scratch_ref.build(SCRATCH)
    path = os.path.join(SCRATCH, "pyfasst", "tftransforms", "minqt.py")
    with open(path) as fh:
        src = fh.read()
    for pat, rep in EXTRA:
        src, n = re.subn(pat, rep, src)
        assert n == 1, (pat, n)
    with open(path, "w") as fh:
        fh.write(src)
    sys.path.insert(0, SCRATCH)


def main():
    import warnings
    warnings.simplefilter('ignore')
    scratch()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    if not hasattr(np, 'complex'):
        np.complex = complex
    import pyfasst.tftransforms.minqt as M
    import cqt_cells_ref as C
    out = {}
    for name in sorted(C.CASES):
        kind, kw, _ = C.CASES[name]
        x = C.signal(name)
        t = (M.CQTransfo if kind == 'cqt' else M.MinQTransfo)(**kw)
        assert t.perfRast == 0
        t.computeTransform(x)
        assert not hasattr(t, '_spCQT')
        k = t.cqtkernel
        out[name + '_x'] = x
        out[name + '_scalars'] = np.array([k.atomHOP, k.first_center, k.winNr, k.fftHOP, k.FFTLen,
                                           t.octaveNr], dtype=np.float64)
        out[name + '_nframes'] = np.array(t.nframes)
        for key, cell in t.cellCQT.items():
            out['%s_cell%s' % (name, '%d' % key if key != 'linear' else '_linear')] = np.array(cell)
        sp = np.array(t.transfo)
        out[name + '_sp'] = sp
        out[name + '_y'] = np.array(t.invertTransform())
        out[name + '_tstamps'] = np.array(t.time_stamps)
        out[name + '_fstamps'] = np.array(t.freq_stamps)
        print(name, 'scalars', out[name + '_scalars'], 'nframes', out[name + '_nframes'],
              'sp', sp.shape)
        if name in C.ROUNDTRIP:
            new = C.modify(name, sp, int(k.bins))
            t.transfo = new
            for key, cell in t.cellCQT.items():
                out['%s_rt_cell%s' % (name, '%d' % key if key != 'linear' else '_linear')] = np.array(cell)
            out[name + '_rt_y'] = np.array(t.invertTransform())
        del t.transfo
        try:
            t.transfo
            out[name + '_del'] = np.array(0)
        except AttributeError:
            out[name + '_del'] = np.array(1)
    fn = os.path.join(HERE, "cqt_cells.npz")
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
