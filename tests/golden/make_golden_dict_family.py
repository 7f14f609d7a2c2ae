"""Generate tests/golden/dict_family.npz by running the REFERENCE's own
SeparateLeadStereo/separateLeadFunctions.py (the scratch py2->py3 translation
built by oracle/make_scratch_ref.py, as tests/golden/make_golden_sigtools.py
does):

    python tests/golden/make_golden_dict_family.py

The cases are those of tests/dict_family_ref.py:

  odgd_<case>_odgd, _spec     generate_ODGD_spec / generate_ODGD_spec_inharmo
  chirp_<case>_odgd, _spec    generate_ODGD_spec_chirped
  wf0_<case>_F0Table, _WF0    generate_WF0_chirped (loadWF0=False, in a scratch
                              working directory: it writes its cache file there)
  minqt_F0Table, minqt_WF0, minqt_cfg
                              generate_WF0_MinQT_chirped on the smallest MinQT
                              geometry of tests/golden/wf0_cqt.npz, if the
                              scratch translation runs it (`minqt_ran` says so)

Numbers only.  The reference text is not patched beyond make_scratch_ref.py's
list.  As in make_golden_sigtools.py, the module's own `np` name gets a zeros()
that truncates a float dimension as the NumPy of the reference's time did
(np.zeros([Nfft, numberElementsInWF0]), :320, with numberOfF0 = np.ceil(...)).
make_scratch_ref.py's array-window patch also reaches generate_ODGD_spec_inharmo,
which therefore accepts an array here; no case uses that.
"""
import contextlib
import io
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"
WORK = "/tmp/golden_dict_family"


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
    from pyfasst.SeparateLeadStereo import separateLeadFunctions as slf
    import dict_family_ref as D
    slf.np = _OldNumpy(np)
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK)
    os.chdir(WORK)
    out = {}
    sink = io.StringIO()
    for name in sorted(D.ODGD_CASES):
        odgd, spec = D.run_odgd_case(name, slf)
        out['odgd_%s_odgd' % name], out['odgd_%s_spec' % name] = odgd, spec
    for name in sorted(D.CHIRP_CASES):
        odgd, spec = D.run_chirp_case(name, slf)
        out['chirp_%s_odgd' % name], out['chirp_%s_spec' % name] = odgd, spec
    for name in sorted(D.WF0_CASES):
        with contextlib.redirect_stdout(sink):
            F0Table, WF0 = slf.generate_WF0_chirped(loadWF0=False, **D.WF0_CASES[name])
        out['wf0_%s_F0Table' % name], out['wf0_%s_WF0' % name] = F0Table, WF0
    g = np.load(os.path.join(HERE, "wf0_cqt.npz"))
    fs, nft, fmin, fmax, bins, minF0, maxF0, stepNotes, perF0 = g['cfg_m1']
    out['minqt_cfg'] = g['cfg_m1']
    try:
        from pyfasst.tools.utils import sqrt_blackmanharris
        with contextlib.redirect_stdout(sink):
            F0Table, WF0, _ = slf.generate_WF0_MinQT_chirped(
                minF0, maxF0, cqtfmax=fmax, cqtfmin=fmin, cqtbins=int(bins), Fs=fs, Nfft=int(nft),
                stepNotes=stepNotes, lengthWindow=int(nft), perF0=int(perF0), loadWF0=False,
                cqtWinFunc=sqrt_blackmanharris)
        out['minqt_F0Table'], out['minqt_WF0'] = F0Table, WF0
        out['minqt_ran'] = np.array(1)
    except Exception as e:       # recorded in minqt_ran
        print("generate_WF0_MinQT_chirped does not run in the scratch translation: %r" % (e,))
        out['minqt_ran'] = np.array(0)
    fn = os.path.join(HERE, "dict_family.npz")
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
