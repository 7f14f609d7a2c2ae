"""Generate tests/golden/spatial_pkg.npz by running the REFERENCE's own
spatial/steering_vectors.py and spatial/dirdiag.py (the scratch py2->py3
translation built by oracle/make_scratch_ref.py, as the other generators do):

    python tests/golden/make_golden_spatial_pkg.py

The reference's steering_vectors.py uses three names it never defines.  They
are bound in that module's namespace before anything is called, and nothing
else of it is touched:

  * `np`             NumPy (audioModel.py, where its far-field functions were
                     cut from, has `import numpy as np`)
  * `soundCelerity`  340. (audioModel.py:63)
  * `inv_mat`        tools.signalTools.inv_herm_mat_2d (called with its
                     signature and its three return values)

After make_scratch_ref.py's own list, one mechanical substitution is made in
the scratch copy: `nfreqs = nft / 2 + 1` -> `nft // 2 + 1` (py2 integer
division, steering_vectors.py:137).  dirdiag.py imports matplotlib at module
level and calls plt.draw() whatever `doplot` is; both are stubbed with empty
modules, and every call passes doplot=None.

Numbers only: none of the reference's text is kept.  The inputs are those of
tests/spatial_pkg_ref.py; the keys are listed by tests/test_spatial_pkg_ref_golden.py.
"""
import os
import re
import shutil
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCRATCH = "/tmp/pyfasst_scratch"

PATCHES = [
    (r"nfreqs = nft / 2 \+ 1", "nfreqs = nft // 2 + 1"),
]


def patch_scratch():
    path = os.path.join(SCRATCH, "pyfasst", "spatial", "steering_vectors.py")
    orig = path + ".orig"
    if not os.path.exists(orig):
        shutil.copy(path, orig)
    src = open(orig).read()
    for pat, rep in PATCHES:
        src, n = re.subn(pat, rep, src)
        if n == 0:
            raise RuntimeError("patch had no effect: " + pat)
    with open(path, "w") as fh:
        fh.write(src)


def stub_matplotlib():
    mpl = types.ModuleType("matplotlib")
    plt = types.ModuleType("matplotlib.pyplot")
    plt.draw = lambda *a, **k: None
    mpl.pyplot = plt
    tk = types.ModuleType("mpl_toolkits")
    m3 = types.ModuleType("mpl_toolkits.mplot3d")
    m3.Axes3D = object
    tk.mplot3d = m3
    sys.modules.update({"matplotlib": mpl, "matplotlib.pyplot": plt, "mpl_toolkits": tk,
                        "mpl_toolkits.mplot3d": m3})


def outcome(fn):
    """(0, result) or (1, None) when the reference raises ValueError"""
    try:
        return 0, fn()
    except ValueError as e:
        print("   ValueError:", str(e).splitlines()[0])
        return 1, None


def main():
    import warnings
    warnings.simplefilter('ignore')
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, REPO)
    import make_scratch_ref
    if not os.path.isdir(os.path.join(SCRATCH, "pyfasst")):
        make_scratch_ref.build(SCRATCH)
    patch_scratch()
    stub_matplotlib()
    sys.path.insert(0, SCRATCH)
    import numpy as np
    if not hasattr(np, 'complex'):
        np.complex = complex
    import pyfasst.spatial.steering_vectors as sv
    import pyfasst.tools.signalTools as st
    sv.np = np
    sv.soundCelerity = 340.
    sv.inv_mat = st.inv_herm_mat_2d
    import pyfasst.spatial.dirdiag as dd
    import spatial_pkg_ref as S

    out = {}
    for name, nch in S.ULA_CASES.items():
        for i, th in enumerate(S.ULA_THETAS):
            out['ula_%s_%d' % (name, i)] = sv.gen_steer_vec_far_src_uniform_linear_array(
                S.FREQS33, nch, th, S.ULA_DIST)
    out['acous'] = sv.gen_steer_vec_acous(S.FREQS33, S.ACOUS_DIST)

    for name in sorted(S.DD_CASES):
        Cx, kw = S.dd_input(name)
        with np.errstate(all='ignore'):
            raised, res = outcome(lambda: sv.dir_diag_stereo(Cx, **kw))
        out['dd_%s_raised' % name] = np.array(raised)
        print("dir_diag_stereo", name, "raised" if raised else "returned")
        if not raised:
            out['dd_%s_diagram' % name], out['dd_%s_theta' % name] = res
            out['dd_%s_mean' % name] = S.cx_tmean(Cx)   # the planes' means, NumPy's own

    for name in sorted(S.MVDR_CASES):
        t, i = S.mvdr_input(name)
        out['mvdr_%s' % name] = dd.make_MVDR_filter_target(t, i)
    for name, (t, i, exc) in sorted(S.mvdr_bad_inputs().items()):
        try:
            dd.make_MVDR_filter_target(t, i)
            raise RuntimeError("the reference accepted the bad input " + name)
        except exc as e:
            out['mvdr_bad_%s' % name] = np.array(type(e).__name__ + ": " + str(e))

    fr, th, A = dd.generate_steer_vec_thetas(**S.SVT_KW)
    out['svt_freqs'], out['svt_thetas'], out['svt_A'] = fr, th, A
    fr2, th2, A2, Raa = dd.generate_steer_vec_thetas(computeRaa=True, **S.SVT_KW)
    assert np.array_equal(A, A2)
    out['svt_Raa'] = Raa

    for n in S.ULAD_SENSORS:
        kw = dict(S.ULAD_KW, n_sensors=n, doplot=None)
        th, fr, d0 = dd.directivity_filter_diagram_ULA(theta_filter=np.pi / 4., **kw)
        out['ulad_%d_thetas' % n], out['ulad_%d_freqs' % n], out['ulad_%d_none' % n] = th, fr, d0
        out['ulad_%d_given' % n] = dd.directivity_filter_diagram_ULA(
            w_filter=S.ulad_filter(n), **kw)[2]
        try:
            dd.directivity_filter_diagram_ULA(w_filter=S.ulad_filter(n)[:, :-1], **kw)
            raise RuntimeError("the reference accepted a filter of the wrong shape")
        except ValueError as e:
            out['ulad_%d_bad' % n] = np.array(str(e))

    fn = os.path.join(HERE, "spatial_pkg.npz")
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
