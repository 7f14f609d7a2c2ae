"""The GEM runs of tests/test_gpu_em_split.py, tests/test_gpu_em_split_more.py
and tests/golden/make_golden_em_split.py: one model per launch path of the EM
engine's phase units, F = 40 bins x T = 70 frames (3 bin tiles and 5 frame
tiles, both ragged), 3 iterations from seeded parameters."""
import numpy as np

F, T, N_ITER = 40, 70, 3

# name: (K per source, ranks, 'conv' per source); what else a case sets is in build()
CASES = {
    "a": ([8, 8], [1, 1], [True, True]),           # single pass, rank-1 arm, both images, fused tail + prep
    "b": ([20, 20, 20], [1, 2, 1], [False] * 3),   # general ranks, k_mix_inst, k_inst_A, one spatial fixed
    "c": ([40] * 4, [2] * 4, [True] * 4),          # rank-2 arm, k_fw_*, unfused launch_renorm
    "d": ([100, 100], [1, 1], [True, True]),       # KP = 128 arms, fused tail without prep
    "e": ([8] * 9, [1] * 9, [True] * 9),           # k_egen_fused<4>
    "f": ([40] * 9, [1] * 9, [True] * 9),          # k_egen_point<16>, k_egen_stats
    "g": ([12, 12], [1, 1], [True, True]),         # two spectral components on source 0: multi_step
    "h": ([12, 12], [1, 1], [True, True]),         # g with lambdaCorr > 0: LAM arms, one component at a time
    "i": ([12, 12], [1, 1], [True, True]),         # g with a time blob of L = 3 on one block, TB free
    "j": ([8, 8], [1, 1], [True, True]),           # TW_constr GSMM on source 0: launch_tw_constr
}

# the cases of tests/golden/em_split_more.npz (k, l: GEM runs as above; m: run_abi)
MORE_CASES = {
    "k": ([8] * 10, [1] * 10, [True] * 10),        # nacc = 300 statistics, 5 per lane: k_mix<11, 4>
    "l": ([8] * 9, [2] * 9, [True] * 9),           # R = 18 > 16: k_mix<11, 16> and its raised LDS ceiling
    "m": CASES["b"],                               # b's model through the stand-alone ABI paths
}
ALL_CASES = dict(CASES, **MORE_CASES)


def _observation(rng):
    X = rng.standard_normal((2, F, T)) + 1j * rng.standard_normal((2, F, T))
    return np.stack([np.abs(X[0]) ** 2 + 0j, np.abs(X[1]) ** 2 + 0j, X[0] * np.conj(X[1])])


def build(name):
    """A configured engine with the case's observation and parameters."""
    from pyfasst_amd.engine import Engine
    Ks, ranks, conv = ALL_CASES[name]
    rng = np.random.default_rng(1000 + ord(name))
    e = Engine(F, T)
    e.configure(ranks, Ks, conv)
    e.set_cx(_observation(rng))
    for j, (K, r, cv) in enumerate(zip(Ks, ranks, conv)):
        shape = (r, 2, F) if cv else (2, r)
        e.set_spatial(j, rng.standard_normal(shape) + 1j * rng.standard_normal(shape),
                      free=not (name in "bm" and j == 1))
        fw_free = name == "c" and j == 2
        FW = 0.5 + rng.random((K, K)) if fw_free else np.eye(K)
        e.set_spectral(j, 0.5 + rng.random((F, K)), FW, 0.5 + rng.random((K, T)), True, True, fw_free)
    if name in "ghi":
        e.set_blocks(0, [0, 5, 12], [1, 1], [0, 0], [1, 1])
    if name == "h":
        e.set_corr(0.1, [0, 0, 1], [0, 1, 0])
    if name == "i":
        e.set_tb(0, 1, 0.5 + rng.random((7, 3)), 0.5 + rng.random((3, T)), tb_free=True)
    if name == "j":
        e.set_tw_constr(0, "GSMM", 0.5 + rng.random((8, T)), None, dp_free=True)
    return e


def _params(e, name):
    """{array name: value}: FB, FW, TW and the mixing parameters of every source."""
    Ks, ranks, conv = ALL_CASES[name]
    out = {}
    for j, (K, r, cv) in enumerate(zip(Ks, ranks, conv)):
        for key, v in zip(("FB", "FW", "TW"), e.get_spectral(j, K)):
            out["%s_%s%d" % (name, key, j)] = v
        out["%s_mix%d" % (name, j)] = e.get_spatial(j, (r, 2, F) if cv else (2, r))
    if name == "i":
        out["i_tbTW"], out["i_tbTB"] = e.get_tb(0, 1, 7, 3)
    return out


def _launches(e):
    """Timed launches per kernel slot, in the order of fasst_kernel_name."""
    from pyfasst_amd._lib import lib
    times = e.kernel_times()
    names = [lib.fasst_kernel_name(i).decode() for i in range(32)]
    return np.array([times.get(n, (0.0, 0))[1] for n in names], dtype=np.int64)


def run(name, profile=False):
    """{array name: value} after N_ITER iterations: FB, FW, TW and the mixing
    parameters of every source, the per-iteration log-likelihoods.  profile:
    with the per-kernel timing events on, and `<name>_launches` added."""
    e = build(name)
    try:
        if profile:
            e.set_profiling(True)
        ll, done, mask = e.run(np.full((N_ITER, F), 1e-3), 1.0)
        out = {"%s_loglik" % name: np.array(ll), "%s_done_mask" % name: np.array([done, mask])}
        out.update(_params(e, name))
        if profile:
            out["%s_launches" % name] = _launches(e)
        return out
    finally:
        e.close()


def run_abi(name="m"):
    """The stand-alone ABI paths on the case's model, no GEM iteration:
    renormalize(), spectral_update(hat_W, 1.0) with a seeded positive hat_W,
    renormalize() again.  {array name: value}: the parameters and both masks."""
    e = build(name)
    try:
        hat_W = 0.5 + np.random.default_rng(2000 + ord(name)).random((len(ALL_CASES[name][0]), F, T))
        m0 = e.renormalize()
        e.spectral_update(hat_W, 1.0)
        m1 = e.renormalize()
        out = {"%s_masks" % name: np.array([m0, m1])}
        out.update(_params(e, name))
        return out
    finally:
        e.close()
