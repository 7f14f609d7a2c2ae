"""Generate tests/golden/slicq_<case>*.npz from the reference's sliced NSGT.

TEST INFRASTRUCTURE ONLY; runs on the CPU in the build container.  The
reference is imported from the scratch Python-3 translation that
oracle/make_scratch_ref.py builds, with the one fix of the in-place integer
clip that tests/golden/make_golden_nsgt.py applies (and applied the same way,
by that module's scratch()); nothing of it is copied here.

Each fixture holds data only.  slicq_<case>.npz: M, nn, rfbas, the window
start bins, the lengths of the kept bands, the concatenated windows of the
bands DC .. Nyquist (g_half; the mirrored bands repeat them) and all dual
windows gd.  The small cases add every slice's concatenated coefficients
(coef [nslices, coef_len]) and the reconstruction cut to the signal's length
(rec).  The big cases would pass the size limit of a committed file in one
piece: slicq_<case>.npz holds the planner and the last slice's coefficients
(c_last), slicq_<case>_coef.npz the first two slices (coef [2, coef_len]),
slicq_<case>_rec.npz the reconstruction.  The input signals are
tests/slicq_ref.py's signal(case).

Usage:  python tests/golden/make_golden_slicq.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))


def main():
    import make_golden_nsgt
    make_golden_nsgt.scratch()
    import slicq_ref as SR
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from pyfasst.tftransforms.nsgt import fscale, slicq
    for name, c in SR.CASES.items():
        scale = fscale.OctScale(c["fmin"], c["fmax"], c["bins"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = slicq.NSGT_sliced(scale, c["sl_len"], c["tr_area"], c["fs"], **SR.options(c))
            x = SR.signal(name)
            slices = [list(cs) for cs in t.forward((x,))]
            lens = [len(b) for b in slices[0]]
            coef = [np.concatenate(cs) for cs in slices]
            rec = np.concatenate([np.asarray(b) for b in t.backward(slices)])
        rec = rec[:len(x)]
        err = np.max(np.abs(rec - x)) / np.max(np.abs(x))
        nh = len(t.g) // 2 + 1
        plan = dict(M=np.asarray(t.M), nn=int(t.nn), rfbas=np.asarray(t.rfbas),
                    start=np.array([w[0] for w in t.wins]), lens=np.array(lens),
                    g_half=np.concatenate(t.g[:nh]), gd=np.concatenate(t.gd), nslices=len(coef))
        for k in range(nh, len(t.g)):   # what g_half leaves out is a repetition
            assert np.array_equal(t.g[k], t.g[len(t.g) - k])
        out = os.path.join(HERE, "slicq_%s.npz" % name)
        sizes = []
        if c.get("big"):
            np.savez_compressed(out, c_last=coef[-1], **plan)
            for suffix, data in (("coef", dict(coef=np.array(coef[:2]))), ("rec", dict(rec=rec))):
                path = os.path.join(HERE, "slicq_%s_%s.npz" % (name, suffix))
                np.savez_compressed(path, **data)
                sizes.append(os.path.getsize(path))
        else:
            np.savez_compressed(out, coef=np.array(coef), rec=rec, **plan)
        sizes.insert(0, os.path.getsize(out))
        assert max(sizes) < (1 << 20), sizes
        print("%-8s slices %3d bands %3d coef_len %6d M %d..%d round trip %.1e  KB %s" % (
            name, len(coef), len(t.g), sum(lens), t.M.min(), t.M.max(), err,
            " ".join("%.0f" % (s / 1024.) for s in sizes)))


if __name__ == "__main__":
    main()
