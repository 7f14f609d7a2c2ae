"""Generate tests/golden/nsgt_<case>.npz from the reference's nsgt package.

TEST INFRASTRUCTURE ONLY; runs on the CPU in the build container.  The
reference is imported from the scratch Python-3 translation that
oracle/make_scratch_ref.py builds; nothing of it is copied here.  Beyond that
recipe the scratch copy needed one mechanical fix, applied to the scratch file
only:

  tftransforms/nsgt/nsgfwin_sl.py   the in-place clip of the integer M against
      (min_win, inf) -- NumPy 2 refuses to cast inf into an integer array --
      becomes the in-place maximum with min_win (every occurrence).

Each fixture holds data only: the input signal, M, nn, rfbas, the
concatenated windows g and duals gd, the window start bins, the concatenated
forward coefficients and the reconstruction.

Usage:  python tests/golden/make_golden_nsgt.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scratch():
    import make_scratch_ref
    dest = make_scratch_ref.build()
    path = os.path.join(dest, "pyfasst", "tftransforms", "nsgt", "nsgfwin_sl.py")
    # the one statement of the planner that clips in place: keep its
    # indentation, replace the call
    lines = open(path).read().split("\n")
    hits = [i for i, ln in enumerate(lines) if ln.strip().startswith("N.clip(")]
    assert hits
    for i in hits:
        indent = lines[i][:len(lines[i]) - len(lines[i].lstrip())]
        lines[i] = indent + "N.maximum(M, min_win, out=M)"
    open(path, "w").write("\n".join(lines))
    sys.path.insert(0, dest)


def main():
    scratch()
    import nsgt_ref as NR
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from pyfasst.tftransforms.nsgt import cq, fscale, nsgfwin_sl
    for name, c in NR.CASES.items():
        if c["kind"] == "oct":
            scale = fscale.OctScale(c["fmin"], c["fmax"], c["bins"])
        else:
            scale = fscale.MelScale(c["fmin"], c["fmax"], c["bnds"])
        kw = dict(real=c["real"], matrixform=c.get("matrixform", False),
                  reducedform=c.get("reducedform", 0), multichannel="nch" in c)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            t = cq.NSGT(scale, c["fs"], c["Ls"], **kw)
            f, q = scale()
            _, rfbas, _ = nsgfwin_sl.nsgfwin(f, q, c["fs"], c["Ls"], sliced=False, dowarn=False)
        qwarn = [str(w.message) for w in caught if "Q-factor" in str(w.message)]
        x = NR.signal(name)
        coef = t.forward(x)
        rec = np.asarray(t.backward(coef))
        chans = coef if "nch" in c else [coef]
        flat = np.array([np.concatenate(ch) for ch in chans])
        out = os.path.join(HERE, "nsgt_%s.npz" % name)
        np.savez_compressed(out, x=x, M=np.asarray(t.M), nn=int(t.nn), rfbas=rfbas,
                            g=np.concatenate(t.g), gd=np.concatenate(t.gd),
                            start=np.array([w[0] for w in t.wins]),
                            lens=np.array([len(b) for b in chans[0]]), coef=flat, rec=rec,
                            q_warned=len(qwarn))
        print("%-9s nn %6d bands %4d Mmax %6d q-warning %d  %6.1f KB" % (
            name, t.nn, len(t.g), t.M.max(), len(qwarn), os.path.getsize(out) / 1024.))


if __name__ == "__main__":
    main()
