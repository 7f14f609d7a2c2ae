"""Secondary benchmarks of the §8 rows next to the headline (bench.py):

  --workload simm   Stereo_SIMM iterations/s at config 5 (F=2049, T=20000,
                    NF0=1092, P=30, K=4, R=40), SIMM.py:613-941
  --workload nmf    NMF_decomposition iterations/s at config 2 (F=1025,
                    T=2000, K=64), tools/nmf.py:34-59
  --workload cqt    MinQT front end (tftransforms/minqt.py:471-646, 1410-1450)
                    as FASST builds it at 44.1 kHz (transf='mqt', wlen 4096,
                    hop 512: FFTLen 8192, 5 octaves x 48 bins + 1980 linear
                    bins) on a signal of T = 10000 STFT frames (the C3 clip
                    length): forward and inverse transforms/s, device time
  --workload wf0    SIMM source dictionary generate_WF0_TR_chirped at config
                    5 (44.1 kHz, NFT 4096, 1092 KLGLOTT88 combs, STFT middle
                    frame): device time per dictionary
  --workload separate_cqt  separation and front end of a MinQT model at the C3
                    clip length: the device-resident calls against the
                    host-side route they replace (profiles/cqt_resident_bench.jsonl)
  --workload spatial  the time-invariant spatial filter at C3
                    (separate_spatial_filter_comp, audioModel.py:891-1061):
                    per-bin gains + the 2 J iSTFTs with the gain applied on
                    load (fasst_spatial_filter_waveforms), host-inclusive
  --workload hmm    the C3 model (bench.py build_model) with every source's
                    time weights SHMM at K = 32 (TW_constr, audioModel.py:
                    1728-1928): ms per GEM iteration, and the two kernels of
                    the discrete-state TW step from fasst_kernel_times
  --workload sf     one GEM iteration of the source / filter model
                    (multiChanSourceF0Filter's default shape: 3 components,
                    the F0 dictionary of minF0=39 .. maxF0=2000 at
                    stepnoteF0=16 plus one column, 20 filter basis functions
                    with 4 weights) at C3's signal size, on the engine (the
                    class surface takes Kb <= 128); with
                    --sparsity L also ms per iteration through sf_run_sparse
                    (both source / filter components reweighed over L frames,
                    sigma from K^2 to 9) and the device time of its two kernels
  --workload sfnmf  SFNMF_decomp_init (tools/nmf.py:161-360) at F = 2049,
                    N = 10000 on the default F0 dictionary's width K = 1093,
                    Kf = 10, Kr = 2: ms per iteration (sfnmf_run), and the
                    CPU restatement's one iteration at the same size
  --workload stereo_nmf  stereo_NMF (SIMM.py:945-1104) at F = 2049, N = 10000,
                    R = 40 (--steps 20): ms per iteration (snmf_run), the same
                    with the error vector, the IS-NMF engine at K = 40 and 48
                    in the same process, and the CPU restatement's one
                    iteration at the same size
  --workload sigtools  tools/signalTools.py: prinComp2D at F = 2049, N = 10000,
                    neighborNb = 20; harmonicSum at F = 2049, T = 10000 on the
                    default F0 grid; medianFilter at 3 rows of N = 10000,
                    length = 10: device ms (HIP events), host-inclusive ms,
                    and the CPU restatement once per case
  --workload demix  DEMIX (demixTF.py) at F = 1025, N = 5002 frames (5000 hops
                    of 1024 samples at 44.1 kHz, wlen = 2048), neighbors = 20,
                    three delayed sources (--steps 3): device ms of the
                    feature stage and per clustering round, the two mask
                    passes' bytes per second, host-inclusive comp_clusters()
                    and refine_clusters(), and the restatement once
  --workload wf0_chirped  generate_WF0_chirped at the reference's default grid
                    (39-2000 Hz, stepNotes 16, 44.1 kHz, Nfft = lengthWindow =
                    2048, perF0 1: 1092 columns): device time of the one
                    dict_odgd launch, host-inclusive time, and the restatement
                    on the host (profiles/dict_family_bench.jsonl)
  --workload dirdiag  dir_diag_stereo (spatial/steering_vectors.py:76-160) at
                    F = 2049, T = 10000, ntheta = 512: device time per kernel,
                    the resident and the host-array route
                    (profiles/dirdiag_bench.jsonl)
  --workload nsgt   CQ_NSGT (tftransforms/nsgt) of 100 s at 44.1 kHz, 48 bins per
                    octave: forward / backward device ms, the whole-signal FFT's
                    share of the HBM copy rate, against the NumPy restatement.
  --workload slicq  CQ_NSGT_sliced (tftransforms/slicq) of the same 100 s in
                    slices of 65536 samples: forward / backward device ms, the
                    generators' host-inclusive ms, the round trip, the
                    whole-signal CQ_NSGT alongside (profiles/slicq_bench.jsonl)
  --workload viterbi  melody tracking (_tracking.pyx:11-93) at config 5:
                    S = 1092 F0 states, N = 20000 frames (runViterbi's
                    transitions, stepNotes 16): tracks/s, device time

Inputs are synthetic and resident in HBM before the timed region; the timed
region is `steps` iterations of the update loop (simm_run / nmf_run, which
synchronise at the end).  Prints one JSON line.  Not part of the driver
contract; the headline metric is bench.py's.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 78.6e12


NO_CPU = False


def bench_simm(steps, warmup, F=2049, N=20000, NF0=1092, P=30, K=4, R=40, seed=0):
    from pyfasst_amd import _lib
    from pyfasst_amd.SeparateLeadStereo.SIMM.SIMM import _SimmContext, _c
    rs = np.random.RandomState(seed)
    SXR = rs.gamma(0.8, 1.0, size=(F, N))
    SXL = rs.gamma(0.8, 1.0, size=(F, N))
    WF0 = rs.gamma(1.0, 1.0, size=(F, NF0))
    WG = rs.gamma(1.0, 1.0, size=(F, P))
    HG, HPHI, HF0 = np.abs(rs.randn(P, K)), np.abs(rs.randn(K, N)), np.abs(rs.randn(NF0, N))
    HM, WM = np.abs(rs.randn(R, N)), np.abs(rs.randn(F, R))
    ctx = _SimmContext(F, N, NF0, P, K, R, True, _lib.default_device())
    _lib.check(_lib.lib.simm_set_data(ctx.ptr, _lib.dptr(SXR), _lib.dptr(SXL), _lib.dptr(WF0),
                                      _lib.dptr(WG)), "set_data")
    alpha, bR = np.array([.5, .5]), rs.rand(R)
    _lib.check(_lib.lib.simm_set_params(ctx.ptr, *[_lib.dptr(_c(a)) for a in
                                                   (HG, HPHI, HF0, HM, WM, alpha, bR)], None),
               "set_params")
    if warmup:
        _lib.check(_lib.lib.simm_run(ctx.ptr, warmup, 1.0, 1, None), "run")
    t0 = time.perf_counter()
    _lib.check(_lib.lib.simm_run(ctx.ptr, steps, 1.0, 1, None), "run")
    dt = time.perf_counter() - t0
    # GEMM flops per iteration: WF0^T{num,den} (2), SF0 recompute (1) on F x NF0 x N;
    # the R-sized products (HM: 4, WM: 4, beta: 4, SM refreshes: 2 x 3) on F x R x N
    flops = 2.0 * F * N * (3 * NF0 + 18 * R)
    achieved = flops / (dt / steps) / 1e12
    # CPU baseline: the oracle restatement (SIMM.py's operation order), ONE
    # iteration at the full size (all N frames: no scaling)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import simm_ref
    n_cpu = N
    np.random.seed(1)
    t1 = time.perf_counter()
    if not NO_CPU:
        simm_ref.stereo_simm(SXR, SXL, WF0, WG, K, R, numberOfIterations=1)
    cpu_s = max(time.perf_counter() - t1, 1e-9)
    return {"metric": "Stereo_SIMM iterations/sec (config 5)", "value": round(steps / dt, 4),
            "unit": "SIMM it/s", "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
            "warmup": warmup, "dtype": "f64", "data": "synthetic gamma spectrograms, RandomState(0)",
            "config": {"workload": "Stereo_SIMM F=%d N=%d NF0=%d P=%d K=%d R=%d" % (F, N, NF0, P, K, R)},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": FP64_PEAK / 1e12,
                         "unit": "TFLOP/s", "frac": round(achieved * 1e12 / FP64_PEAK, 4),
                         "traffic": None, "scope": "whole iteration, GEMM flops 2FN(3 NF0 + 18 R)"},
            "gemm_tflops_per_s": round(achieved, 2),
            "cpu_baseline": {"value": round(1.0 / cpu_s, 5), "unit": "SIMM it/s", "cores": _blas_threads(),
                             "kind": "port", "sample": "oracle/simm_ref.py stereo_simm, 1 iteration "
                             "at the full size, %d frames (%.2f s)" % (n_cpu, cpu_s)},
            "reference_cpu": "14.27 s/iter = 0.070 it/s (BASELINE/SURVEY §6, measured on CPU)"}


def _blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return int(max([p.get('num_threads', 1) for p in threadpool_info()] + [1]))
    except Exception:
        return 1


def bench_separate(steps, warmup):
    """Wiener separation + iSTFT at C3 (audioModel.py:1088-1233): the device-
    resident path (fasst_separate_waveforms, only the 8 waveforms cross PCIe)
    vs the images path (fasst_wiener_images: J x 2 x F x T complex images to
    the host, the per-image iSTFT after).  Host-inclusive wall times."""
    sys.path.insert(0, ROOT)
    import bench as B
    m = B.build_model(seed=0, device=0)
    eng = m._engine
    m._upload()
    nfft, hop = 4096, 512
    w = np.hanning(nfft)
    psd = np.full(m.nbFreqsSigRepr, 1e-6)
    for _ in range(max(warmup, 1)):
        eng.separate_waveforms(psd, w, w, nfft, hop)
    t0 = time.perf_counter()
    for _ in range(steps):
        Y = eng.separate_waveforms(psd, w, w, nfft, hop)
    dt = (time.perf_counter() - t0) / steps
    eng.wiener_images(psd)
    t1 = time.perf_counter()
    for _ in range(steps):
        S = eng.wiener_images(psd)
    di = (time.perf_counter() - t1) / steps
    J = Y.shape[0]
    # front end as FASST runs it (comp_transf_Cx, audioModel.py:250-302):
    # fasst_set_audio uploads the 2-channel signal, STFTs it on the device and
    # builds Cx there (the channel STFTs stay resident for the separation)
    L = hop * (m.nbFramesSigRepr - 2)
    x = np.random.RandomState(0).randn(L, 2)
    eng.set_audio(x, w, nfft, hop)
    t2 = time.perf_counter()
    for _ in range(steps):
        eng.set_audio(x, w, nfft, hop)
    ds = (time.perf_counter() - t2) / steps
    return {"metric": "FASST separation (Wiener images + iSTFT) per clip, host-inclusive",
            "value": round(dt * 1e3, 3), "unit": "ms", "higher_is_better": False,
            "steps": steps, "warmup": warmup, "dtype": "f64",
            "data": "synthetic C3 model (bench.py build_model, seed 0)",
            "config": {"workload": "J=%d sources x 2 channels, F=%d, T=%d, nfft %d hop %d"
                                   % (J, m.nbFreqsSigRepr, m.nbFramesSigRepr, nfft, hop)},
            "waveform_bytes_to_host": int(Y.nbytes),
            "images_path_ms": round(di * 1e3, 3), "image_bytes_to_host": int(S.nbytes),
            "front_end_ms": round(ds * 1e3, 3), "front_end": "fasst_set_audio: %d x 2 samples -> "
            "resident STFTs + Cx, host-inclusive" % L}


def bench_separate_cqt(steps, warmup, fs=44100, wlen=4096, hop=512, T=10000, J=4, K=32, seed=0):
    """Separation of a MinQT model at the length of the `separate` workload's
    C3 clip: the device-resident call (fasst_separate_waveforms_cqt: the 2 J
    images stay in HBM and go through one batched inverse) against the route
    it replaces (fasst_wiener_images to the host, then 2 J cqt_inverse calls),
    in one session, host-inclusive; beside them the device time of the inverse
    chains (cqt_device_ms) and the same pair for the front end
    (fasst_set_audio_cqt against 2 cqt_forward + fasst_set_stft)."""
    from pyfasst_amd import _lib
    from pyfasst_amd.engine import Engine
    from pyfasst_amd.tftransforms import minqt
    L = hop * (T - 2)
    rs = np.random.RandomState(seed)
    x = rs.randn(L, 2) * (1 + np.sin(np.arange(L) / 7000.0))[:, None]
    x[:, 1] = 0.6 * x[:, 1] + 0.4 * np.roll(x[:, 0], 5)
    t = minqt.MinQTransfo(fmin=25, fmax=18000, bins=48, fs=fs, perfRast=1, linFTLen=wlen,
                          atomHopFactor=hop / float(wlen))
    cqt = t._context()
    F, W = t.prepare_resident(L)
    eng = Engine(F, W)

    def dev_ms():
        f, b = ctypes.c_double(), ctypes.c_double()
        _lib.check(_lib.lib.cqt_device_ms(cqt, ctypes.byref(f), ctypes.byref(b)), "ms")
        return f.value, b.value

    def timed(fn):
        """(median wall ms, median of fn's own return value) over the steps"""
        wall, own = [], []
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            if i >= warmup:
                wall.append(dt * 1e3)
                own.append(r)
        return float(np.median(wall)), float(np.median(own))

    # ---- front end
    def front_new():
        eng.set_audio_cqt(cqt, x)
        return dev_ms()[0]

    def front_old():
        X, ms = [], 0.0
        for c in range(2):
            t.computeTransform(x[:, c])
            ms += dev_ms()[0]
            X.append(t.transfo)
        eng.set_stft(np.array(X))
        return ms
    fo_wall, fo_dev = timed(front_old)
    cx_old = eng.get_cx()
    fn_wall, fn_dev = timed(front_new)
    front_equal = bool(np.array_equal(cx_old, eng.get_cx()))
    del cx_old
    fwd_info = t.batch_info()

    # ---- the model: J 'conv' components of rank 2, K NMF components each
    eng.configure([2] * J, [K] * J, True)
    for j in range(J):
        eng.set_spatial(j, rs.randn(2, 2, F) + 1j * rs.randn(2, 2, F), False)
        eng.set_spectral(j, rs.gamma(1.0, 1.0, (F, K)), np.eye(K), rs.gamma(1.0, 1.0, (K, W)),
                         True, True)
    eng.set_sources(None)
    psd = np.full(F, 1e-6)
    keep = {}

    def sep_new():
        keep['new'] = eng.separate_waveforms_cqt(cqt, psd, L)
        return dev_ms()[1]

    def sep_old():
        S = eng.wiener_images(psd)
        Y, ms = np.empty((J, 2, L)), 0.0
        for n in range(J):
            for c in range(2):
                t.transfo = S[n, c]
                Y[n, c] = t.invertTransform()
                ms += dev_ms()[1]
                del t.transfo
        keep['old'], keep['image_bytes'] = Y, int(S.nbytes)
        return ms
    so_wall, so_dev = timed(sep_old)
    sn_wall, sn_dev = timed(sep_new)
    inv_info = t.batch_info()
    err = float(np.max(np.abs(keep['new'] - keep['old'])) / np.max(np.abs(keep['old'])))
    return {"metric": "MinQT model separation (Wiener images + inverse MinQT) per clip, "
                      "host-inclusive",
            "value": round(sn_wall, 3), "unit": "ms", "higher_is_better": False,
            "steps": steps, "warmup": warmup, "dtype": "f64",
            "data": "synthetic modulated stereo noise, random 'conv' model, RandomState(0)",
            "config": {"workload": "MinQT fs=%d linFTLen=%d hop=%d bins=48 fmin=25: %d samples, "
                                   "spCQT %dx%d, %d octaves; J=%d sources x 2 channels, K=%d"
                                   % (fs, wlen, hop, L, F, W, int(t.octaveNr), J, K)},
            "old_route_ms": round(so_wall, 3),
            "old_route": "fasst_wiener_images + %d x cqt_inverse, host-inclusive" % (2 * J),
            "speedup_vs_old_route": round(so_wall / sn_wall, 2),
            "inverse_device_ms": {"batched": round(sn_dev, 3),
                                  "singles_sum": round(so_dev, 3),
                                  "signals": inv_info[0], "launches": inv_info[1]},
            "waveform_bytes_to_host": int(keep['new'].nbytes),
            "image_bytes_to_host_old_route": keep['image_bytes'],
            "rel_diff_vs_old_route": err,
            "front_end_ms": round(fn_wall, 3), "front_end_old_route_ms": round(fo_wall, 3),
            "front_end_old_route": "2 x cqt_forward to the host + fasst_set_stft, host-inclusive",
            "front_end_device_ms": {"batched": round(fn_dev, 3), "singles_sum": round(fo_dev, 3),
                                    "signals": fwd_info[0], "launches": fwd_info[1]},
            "front_end_cx_bit_equal": front_equal}


def bench_spatial(steps, warmup):
    """The fused spatial filter at C3: the same 2 J iSTFTs as `separate`, no
    per-point Wiener pass and no image planes in HBM; the images path
    (fasst_spatial_filter_images) beside it.  Host-inclusive wall times."""
    sys.path.insert(0, ROOT)
    import bench as B
    m = B.build_model(seed=0, device=0)
    eng = m._engine
    m._upload()
    nfft, hop = 4096, 512
    w = np.hanning(nfft)
    for _ in range(max(warmup, 1)):
        eng.spatial_filter_waveforms(w, w, nfft, hop)
    t0 = time.perf_counter()
    for _ in range(steps):
        Y = eng.spatial_filter_waveforms(w, w, nfft, hop)
    dt = (time.perf_counter() - t0) / steps
    eng.spatial_filter_images()
    t1 = time.perf_counter()
    for _ in range(steps):
        S = eng.spatial_filter_images()
    di = (time.perf_counter() - t1) / steps
    J = Y.shape[0]
    return {"metric": "FASST spatial filter (per-bin gains + gain-on-load iSTFT) per clip, "
                      "host-inclusive",
            "value": round(dt * 1e3, 3), "unit": "ms", "higher_is_better": False,
            "steps": steps, "warmup": warmup, "dtype": "f64",
            "data": "synthetic C3 model (bench.py build_model, seed 0)",
            "config": {"workload": "J=%d sources x 2 channels, F=%d, T=%d, nfft %d hop %d"
                                   % (J, m.nbFreqsSigRepr, m.nbFramesSigRepr, nfft, hop)},
            "waveform_bytes_to_host": int(Y.nbytes),
            "images_path_ms": round(di * 1e3, 3), "image_bytes_to_host": int(S.nbytes)}


def bench_hmm(steps, warmup):
    """C3 with every source SHMM at K = 32: ms per GEM iteration (device
    batch, one host sync), then a profiled batch for the per-kernel times."""
    sys.path.insert(0, ROOT)
    import bench as B
    m = B.build_model(seed=0, device=0)
    for comp in m.spec_comps.values():
        fac = comp['factor'][0]
        fac['TW_constr'] = 'SHMM'
        fac['TW_DP_frdm_prior'] = 'free'
    eng = m._engine
    m._upload()
    F, T = m.nbFreqsSigRepr, m.nbFramesSigRepr
    rows = np.array([m._annealed_psd(0)] * max(steps, warmup, 1), dtype=np.float64)
    eng.run(rows[:max(warmup, 1)], 1.0)
    t0 = time.perf_counter()
    eng.run(rows[:steps], 1.0)
    dt = (time.perf_counter() - t0) / steps
    eng.set_profiling(True)
    eng.run(rows[:steps], 1.0)
    kt = eng.kernel_times()
    eng.set_profiling(False)
    J, K = len(m.spat_comps), m.nbNMFComps
    div_ms = kt.get("k_tw_statediv", (0.0, 0))[0]
    rho_bytes = 8.0 * J * F * T          # one read of rho per source
    return {"metric": "GEM iteration, every source SHMM (discrete-state TW step)",
            "value": round(dt * 1e3, 3), "unit": "ms", "higher_is_better": False,
            "steps": steps, "warmup": warmup, "dtype": "f64",
            "data": "synthetic C3 model (bench.py build_model, seed 0)",
            "config": {"workload": "F=%d T=%d J=%d K=%d SHMM, free transitions" % (F, T, J, K)},
            "k_tw_statediv_ms": round(div_ms, 4),
            "k_tw_decode_ms": round(kt.get("k_tw_decode", (0.0, 0))[0], 4),
            "statediv_hbm_fraction": round(rho_bytes / (div_ms * 1e-3) / 8.0e12, 4)
            if div_ms else None,
            "statediv_logs": int(J) * int(K) * int(F) * int(T),
            "kernel_ms": {k: round(v[0], 4) for k, v in sorted(kt.items())}}


def bench_nmf(steps, warmup, F=1025, N=2000, K=64, seed=0):
    from pyfasst_amd import _lib
    from pyfasst_amd.tools.nmf import _NmfContext
    rs = np.random.RandomState(seed)
    SX = rs.gamma(0.7, 1.0, size=(F, N))
    W = rs.randn(F, K) ** 2
    H = rs.randn(K, N) ** 2
    W /= W.sum(axis=0)
    ctx = _NmfContext(F, N, K, _lib.default_device())
    _lib.check(_lib.lib.nmf_set_data(ctx.ptr, _lib.dptr(SX)), "set_data")
    _lib.check(_lib.lib.nmf_set_params(ctx.ptr, _lib.dptr(W), _lib.dptr(H)), "set_params")
    if warmup:
        _lib.check(_lib.lib.nmf_run(ctx.ptr, warmup, 1, 1), "run")
    t0 = time.perf_counter()
    _lib.check(_lib.lib.nmf_run(ctx.ptr, steps, 1, 1), "run")
    dt = time.perf_counter() - t0
    flops = 2.0 * F * N * K * 6
    achieved = flops / (dt / steps) / 1e12
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import fasst_ref
    n_cpu = 20
    t1 = time.perf_counter()
    if not NO_CPU:
        fasst_ref.nmf_decomp_init(SX, nbComps=K, niter=n_cpu, Winit=W.copy(), Hinit=H.copy())
    cpu_s = max((time.perf_counter() - t1) / n_cpu, 1e-9)
    return {"metric": "NMF_decomposition iterations/sec (config 2)", "value": round(steps / dt, 3),
            "unit": "NMF it/s", "ms_per_step": round(dt / steps * 1e3, 4), "steps": steps,
            "warmup": warmup, "dtype": "f64", "data": "synthetic gamma spectrogram, RandomState(0)",
            "config": {"workload": "IS-NMF F=%d T=%d K=%d" % (F, N, K)},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": FP64_PEAK / 1e12,
                         "unit": "TFLOP/s", "frac": round(achieved * 1e12 / FP64_PEAK, 4),
                         "traffic": None, "scope": "whole iteration, GEMM flops 12FTK"},
            "gemm_tflops_per_s": round(achieved, 2),
            "cpu_baseline": {"value": round(1.0 / cpu_s, 3), "unit": "NMF it/s", "cores": _blas_threads(),
                             "kind": "port", "sample": "oracle/fasst_ref.py nmf_decomp_init, %d "
                             "iterations at the full size" % n_cpu},
            "reference_cpu": "0.0318 s/iter = 31.4 it/s (SURVEY §6, measured on CPU)"}


def _bench_cqt_cells(x, steps, warmup, fs, wlen, hop):
    """The same MinQT with perfRast=0: forward to cells, cells -> raster,
    raster -> cells (the transfo setter) and the inverse from the cells."""
    from pyfasst_amd import _lib
    from pyfasst_amd.tftransforms import minqt
    t = minqt.MinQTransfo(fmin=25, fmax=18000, bins=48, fs=fs, linFTLen=wlen,
                          atomHopFactor=hop / float(wlen))
    ms = {"forward_ms": [], "raster_ms": [], "raster_to_cells_ms": [], "inverse_ms": []}
    for i in range(warmup + steps):
        t.computeTransform(x)
        sp = t.transfo
        t.transfo = sp
        y = t.invertTransform()
        f, b, r, c = (ctypes.c_double() for _ in range(4))
        _lib.check(_lib.lib.cqt_device_ms(t._context(), ctypes.byref(f), ctypes.byref(b)), "ms")
        _lib.check(_lib.lib.cqt_raster_device_ms(t._context(), ctypes.byref(r), ctypes.byref(c)),
                   "ms")
        if i >= warmup:
            for key, v in zip(("forward_ms", "raster_ms", "raster_to_cells_ms", "inverse_ms"),
                              (f, r, c, b)):
                ms[key].append(v.value)
    out = {key: round(float(np.median(v)), 3) for key, v in ms.items()}
    n_cells = sum(c.size for c in t.cellCQT.values())
    # complex128 elements moved at the least: every cell element and every
    # raster element once (the strided gather of raster -> cells touches more
    # cache lines than it uses: at most the whole raster)
    out["cells_bytes"] = 16 * n_cells
    out["raster_bytes"] = 16 * sp.size
    out["raster_gbps_min"] = round(16e-6 * (n_cells + sp.size) / out["raster_ms"], 1)
    out["raster_to_cells_gbps_min"] = round(16e-6 * 2 * n_cells / out["raster_to_cells_ms"], 1)
    out["raster_to_cells_gbps_max"] = round(16e-6 * (n_cells + sp.size) /
                                            out["raster_to_cells_ms"], 1)
    out["roundtrip_rel_err"] = float(np.abs(y - x).max() / np.abs(x).max())
    out["cells"] = "%d octaves + linear, %d elements; raster %dx%d" % (
        int(t.octaveNr), n_cells, sp.shape[0], sp.shape[1])
    return out


def bench_cqt(steps, warmup, fs=44100, wlen=4096, hop=512, T=10000, seed=0):
    from pyfasst_amd import _lib
    from pyfasst_amd.tftransforms import minqt
    L = hop * (T - 2)
    rs = np.random.RandomState(seed)
    x = rs.randn(L) * (1 + np.sin(np.arange(L) / 7000.0))
    t = minqt.MinQTransfo(fmin=25, fmax=18000, bins=48, fs=fs, perfRast=1, linFTLen=wlen,
                          atomHopFactor=hop / float(wlen))
    fwd, inv = [], []
    for i in range(warmup + steps):
        t.computeTransform(x)
        sp = t.transfo
        y = t.invertTransform()
        f, b = ctypes.c_double(), ctypes.c_double()
        _lib.check(_lib.lib.cqt_device_ms(t._context(), ctypes.byref(f), ctypes.byref(b)), "ms")
        if i >= warmup:
            fwd.append(f.value)
            inv.append(b.value)
    k = t.cqtkernel
    fm, im = float(np.median(fwd)), float(np.median(inv))
    cells_run = _bench_cqt_cells(x, steps, warmup, fs, wlen, hop)
    return {"metric": "MinQT forward transforms/sec (device time)", "value": round(1e3 / fm, 3),
            "perfRast0": cells_run,
            "unit": "transforms/s", "forward_ms": round(fm, 3), "inverse_ms": round(im, 3),
            "msamples_per_s_forward": round(L / fm / 1e3, 1), "steps": steps, "warmup": warmup,
            "dtype": "f64", "data": "synthetic modulated noise, RandomState(0)",
            "config": {"workload": "MinQT fs=%d linFTLen=%d hop=%d bins=48 fmin=25: %d samples "
                                   "(T=%d frames), spCQT %dx%d, FFTLen %d, %d octaves, "
                                   "kernel band %s" % (fs, wlen, hop, L, T, sp.shape[0],
                                                       sp.shape[1], int(k.FFTLen),
                                                       int(t.octaveNr), "n/a")},
            "roundtrip_rel_err": float(np.abs(y - x).max() / np.abs(x).max())}


def bench_wf0(steps, warmup):
    import tempfile
    from pyfasst_amd import _lib
    from pyfasst_amd.SeparateLeadStereo import separateLeadFunctions as slf
    from pyfasst_amd.tftransforms.stft import STFT
    from pyfasst_amd.tools.utils import sqrt_blackmanharris
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import dict_ref as D
    os.chdir(tempfile.mkdtemp())
    t = STFT(linFTLen=4096, atomHopFactor=0.25, winFunc=sqrt_blackmanharris, fs=44100)
    ms = []
    for i in range(warmup + steps):
        F0Table, WF0, _ = slf.generate_WF0_TR_chirped(t, 39, 2000, stepNotes=16, loadWF0=False)
        m = ctypes.c_double()
        _lib.lib.dict_last_ms(ctypes.byref(m))
        if i >= warmup:
            ms.append(m.value)
    dm = float(np.median(ms))
    ab = ctypes.c_int()
    _lib.lib.viterbi_fallback_count(ctypes.byref(ab))
    # CPU: the oracle (the reference's outer-product synthesis) on 8 of the 1092 F0s
    idx = np.linspace(0, F0Table.size - 1, 8).astype(int)
    t0 = time.perf_counter()
    for i in idx:
        D.stft_mid_frame_power(D.generate_odgd(F0Table[i], 44100, lengthOdgd=8192), t.window,
                               t.fthop, 4096, 44100)
    cpu_s = (time.perf_counter() - t0) / idx.size * F0Table.size
    partials = sum(int(np.floor(22050.0 / f)) for f in F0Table)
    return {"metric": "SIMM WF0 dictionaries/sec (config 5, device time)",
            "value": round(1e3 / dm, 3), "unit": "dictionaries/s", "device_ms": round(dm, 3),
            "steps": steps, "warmup": warmup, "dtype": "f64",
            "config": {"workload": "generate_WF0_TR_chirped STFT NFT=4096 fs=44100 minF0=39 "
                                   "maxF0=2000 stepNotes=16: %d combs, %d partials, 4096-sample "
                                   "frames" % (F0Table.size, partials)},
            "partial_samples_per_s": round(partials * 4096 / (dm * 1e-3) / 1e9, 2),
            "cpu_baseline": {"value": round(1.0 / cpu_s, 5), "unit": "dictionaries/s",
                             "cores": 1, "kind": "port",
                             "sample": "oracle/dict_ref.py on 8 of the %d F0s, scaled"
                                       % F0Table.size}}


def bench_wf0_chirped(steps, warmup):
    import tempfile
    from pyfasst_amd import _lib
    from pyfasst_amd.SeparateLeadStereo import separateLeadFunctions as slf
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dict_family_ref as D
    os.chdir(tempfile.mkdtemp())
    kw = dict(minF0=39, maxF0=2000, Fs=44100, Nfft=2048, stepNotes=16, lengthWindow=2048, perF0=1)
    ms, host = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        F0Table, WF0 = slf.generate_WF0_chirped(loadWF0=False, **kw)
        dt = time.perf_counter() - t0
        m = ctypes.c_double()
        _lib.lib.dict_last_ms(ctypes.byref(m))
        if i >= warmup:
            ms.append(m.value)
            host.append(dt * 1e3)
    dm = float(np.median(ms))
    # CPU: the restatement (the reference's outer-product synthesis) on 8 of the F0s
    idx = np.linspace(0, F0Table.size - 1, 8).astype(int)
    t0 = time.perf_counter()
    for i in idx:
        D.generate_ODGD_spec(F0Table[i], 44100, lengthOdgd=2048, Nfft=2048,
                             analysisWindowType='hanning')
    cpu_s = (time.perf_counter() - t0) / idx.size * F0Table.size
    partials = sum(int(np.floor(22050.0 / f)) for f in F0Table)
    return {"metric": "generate_WF0_chirped dictionaries/sec (default grid, device time)",
            "value": round(1e3 / dm, 3), "unit": "dictionaries/s", "device_ms": round(dm, 3),
            "host_inclusive_ms": round(float(np.median(host)), 3),
            "steps": steps, "warmup": warmup, "dtype": "f64",
            "config": {"workload": "generate_WF0_chirped fs=44100 Nfft=lengthWindow=2048 minF0=39 "
                                   "maxF0=2000 stepNotes=16 perF0=1: %d combs, %d partials, WF0 "
                                   "%d x %d" % (F0Table.size, partials, WF0.shape[0],
                                                WF0.shape[1])},
            "partial_samples_per_s": round(partials * 2048 / (dm * 1e-3) / 1e9, 2),
            "cpu_baseline": {"value": round(1.0 / cpu_s, 5), "unit": "dictionaries/s",
                             "cores": 1, "kind": "port", "seconds": round(cpu_s, 2),
                             "sample": "tests/dict_family_ref.py generate_ODGD_spec on 8 of the "
                                       "%d F0s, scaled" % F0Table.size}}


def bench_nnls(steps, warmup, frames=1000, seed=0):
    """initHF00='nnls' on one pipeline chunk at config-5 scale: the C5 STFT
    dictionary (1092 combs, F=2049) and 1000 frames of synthetic spectra
    (a few combs + noise), one batched GPU solve per step; the CPU baseline
    is scipy.optimize.nnls (the reference's call) on a sample of frames."""
    import tempfile
    from pyfasst_amd.SeparateLeadStereo import separateLeadFunctions as slf
    from pyfasst_amd.tftransforms.stft import STFT
    from pyfasst_amd.tools.nnls import nnls_columns
    from pyfasst_amd.tools.utils import sqrt_blackmanharris
    os.chdir(tempfile.mkdtemp())
    t = STFT(linFTLen=4096, atomHopFactor=0.25, winFunc=sqrt_blackmanharris, fs=44100)
    F0Table, WF0, _ = slf.generate_WF0_TR_chirped(t, 39, 2000, stepNotes=16, loadWF0=False)
    rs = np.random.RandomState(seed)
    F, n = WF0.shape
    H = np.zeros((n, frames))
    for q in range(frames):
        H[rs.choice(n, 4, replace=False), q] = rs.rand(4)
    SX = WF0.dot(H) + 1e-3 * WF0.max() * rs.rand(F, frames)
    ms = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        X = nnls_columns(WF0, SX)
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    dm = float(np.median(ms))
    out = {"metric": "NNLS frames/sec (initHF00='nnls', one 1000-frame chunk, host-inclusive)",
           "value": round(frames / (dm * 1e-3), 2), "unit": "frames/s", "ms_per_chunk": round(dm, 2),
           "steps": steps, "warmup": warmup, "dtype": "f64",
           "config": {"workload": "nnls(WF0 %d x %d, 1000 frames)" % (F, n)},
           "active_mean": round(float(np.mean(np.sum(X > 0, axis=0))), 1)}
    if not NO_CPU:
        from scipy.optimize import nnls
        t0 = time.perf_counter()
        k = 4
        ref = [nnls(WF0, SX[:, q])[0] for q in range(k)]
        cpu = (time.perf_counter() - t0) / k
        out["vs_scipy"] = {"max_rel": float(max(np.max(np.abs(X[:, q] - ref[q])) /
                                              max(np.max(np.abs(ref[q])), 1e-300)
                                              for q in range(k))),
                           "same_support": bool(all(np.array_equal(X[:, q] > 0, ref[q] > 0)
                                                    for q in range(k)))}
        out["cpu_baseline"] = {"value": round(1.0 / cpu, 3), "unit": "frames/s", "cores": 1,
                               "kind": "reference",
                               "sample": "scipy.optimize.nnls (the reference's call) on 4 frames"}
    return out


def bench_viterbi(steps, warmup, S=1092, N=20000, seed=0):
    from pyfasst_amd import _lib
    from pyfasst_amd.SeparateLeadStereo.tracking._tracking import viterbiTracking
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import viterbi_ref as V
    rs = np.random.RandomState(seed)
    logD = np.log(rs.gamma(0.3, 1.0, size=(S + 1, N)))
    logT, prior = V.melody_transitions(S, 16)
    ms = []
    for i in range(warmup + steps):
        viterbiTracking(S, N, logD, prior, logT)
        m, k = ctypes.c_double(), ctypes.c_int()
        _lib.lib.viterbi_last_timing(ctypes.byref(m), ctypes.byref(k))
        if i >= warmup:
            ms.append(m.value)
    dm = float(np.median(ms))
    ab = ctypes.c_int()
    _lib.lib.viterbi_fallback_count(ctypes.byref(ab))
    # CPU: the oracle restatement of the pyx recursion on a bounded sample
    n_cpu = 40
    t0 = time.perf_counter()
    V.viterbi_tracking(S, n_cpu, logD, prior, logT)
    cpu_s = (time.perf_counter() - t0) / (n_cpu - 1) * (N - 1)
    return {"metric": "Viterbi melody tracks/sec (config 5 size, device time)",
            "value": round(1e3 / dm, 3), "unit": "tracks/s", "device_ms": round(dm, 2),
            "us_per_frame": round(dm * 1e3 / N, 3), "steps": steps, "warmup": warmup,
            "dtype": "f64", "data": "synthetic log-gamma densities, RandomState(0)",
            "config": {"workload": "viterbiTracking S=%d N=%d (max-plus S^2 per frame)" % (S, N)},
            "maxplus_gops": round(float(S) * S * (N - 1) / (dm * 1e-3) / 1e9, 1),
            # persistent launches rerun on the per-frame path (results taken
            # on the slower fallback are identifiable)
            "path_kind": k.value, "persistent_aborts": ab.value,
            "cpu_baseline": {"value": round(1.0 / cpu_s, 5), "unit": "tracks/s", "cores": 1,
                             "kind": "port", "sample": "oracle/viterbi_ref.py, %d frames, "
                             "scaled to N=%d" % (n_cpu, N)}}


COPY_GBS = 6290.0   # the device copy rate profiles/sigtools_bench.jsonl measured


def bench_sf(steps, warmup, F=2049, T=10000, seed=0, sparsity=0):
    """The two-factor path (csrc/fasst_sf.hip) at the reference class's default
    shape: ms per GEM iteration (a host sync per iteration: the restart flags),
    then the launch counts of a profiled iteration.  sparsity = L > 0: the
    same through sf_run_sparse with both source / filter components reweighed,
    in the same session, and the two kernels' device time against TW read
    twice and written once at the measured copy rate."""
    from pyfasst_amd import synthetic
    from pyfasst_amd.engine import Engine
    nf0 = int(np.ceil(12.0 * 16 * np.log2(2000.0 / 39.0)) + 1) + 1     # + the column of ones
    kf, kw, kres = 20, 4, 1
    rs = np.random.RandomState(seed)
    X = synthetic.stereo_mixture(F, T, J=3, K_true=8, rank=1, seed=seed)
    eng = Engine(F, T, 0)
    eng.set_stft(X)
    pos = lambda *shape: 0.75 * np.abs(rs.randn(*shape)) + 0.25
    factors = [[(nf0, nf0, False, False, True), (kf, kw, False, True, True)]] * 2 + \
              [[(kres, kres, True, False, True)]]
    alias = [[(-1, -1, -1), (-1, -1, -1)], [(0, 0, -1), (1, -1, -1)], [(-1, -1, -1)]]
    eng.sf_configure([1, 1, 1], False, factors, alias)
    src, filt = pos(F, nf0), pos(F, kf)
    for j in range(3):
        eng.sf_set_spatial(j, rs.randn(2, 1), True)
    for j in range(2):
        eng.set_factors(j, 0, src, np.eye(nf0), pos(nf0, T))
        eng.set_factors(j, 1, filt, pos(kf, kw), pos(kw, T))
    eng.set_factors(2, 0, pos(F, kres), np.eye(kres), pos(kres, T))
    eng.renormalize()
    psd = np.tile(eng.mix_psd() / 100., (max(steps, warmup, 1), 1))
    eng.run(psd[:max(warmup, 1)], 1.0)
    t0 = time.perf_counter()
    eng.run(psd[:steps], 1.0)
    dt = (time.perf_counter() - t0) / steps
    eng.set_profiling(True)
    eng.run(psd[:1], 1.0)
    kt = eng.kernel_times()
    eng.set_profiling(False)
    gflop = 2.0 * 2 * F * nf0 * T * (3 + 2) / 1e9   # P0 three times, W0^T [rn | rd]: per SF component
    sparse = None
    if sparsity > 0:
        n = max(steps, warmup, 2)
        sig = np.exp(np.log(float(nf0) ** 2) + (np.log(9.0) - np.log(float(nf0) ** 2)) *
                     np.arange(n) / (n - 1.0))
        eng.sf_set_sparsity([sparsity, sparsity, 0])
        eng.sf_run_sparse(psd[:max(warmup, 1)], 1.0, sig[:max(warmup, 1)])
        t0 = time.perf_counter()
        _, done, mask = eng.sf_run_sparse(psd[:steps], 1.0, sig[:steps])
        dts = (time.perf_counter() - t0) / max(done, 1)
        eng.set_profiling(True)
        eng.sf_run_sparse(psd[:1], 1.0, sig[-1:])
        ks = eng.kernel_times()
        eng.set_profiling(False)
        copy_ms = 3.0 * nf0 * T * 8 / (COPY_GBS * 1e9) * 1e3   # per sparse component
        dev = {k: round(float(ks[k][0]), 4) for k in ("k_sf_bary", "k_sf_sparsify")}
        sparse = {"length": sparsity, "sparse_components": 2, "iterations": int(done),
                  "restart_mask": int(mask), "ms_per_iteration": round(dts * 1e3, 3),
                  "ms_per_iteration_without": round(dt * 1e3, 3),
                  "kernel_device_ms_per_launch": dev,
                  "launches_per_iteration": {k: int(ks[k][1]) for k in dev},
                  "reweigh_device_ms_per_iteration": round(2 * sum(dev.values()), 4),
                  "copy_rate_ms_per_component": round(copy_ms, 4),
                  "frac_of_measured_copy_%d" % COPY_GBS: round(copy_ms / sum(dev.values()), 4)}
    return {"metric": "GEM iteration, source / filter model (two-factor path)",
            "value": round(dt * 1e3, 3), "unit": "ms", "higher_is_better": False,
            "steps": steps, "warmup": warmup, "dtype": "f64",
            "data": "synthetic STFT-domain stereo mixture (seed %d), seeded positive factors" % seed,
            "config": {"workload": "F=%d T=%d, 3 components: 2 x (FB %dx%d . I . TW %dxT) * "
                                   "(FB %dx%d . FW %dx%d . TW %dxT) + 1 x NMF K=%d, rank 1 'inst'"
                                   % (F, T, F, nf0, nf0, F, kf, kf, kw, kw, kres)},
            "source_factor_gflop": round(gflop, 1),
            "source_factor_tflops": round(gflop / 1e3 / dt, 2),
            "launches_per_iteration": {k: int(v[1]) for k, v in sorted(kt.items())},
            "sparsity": sparse}


def bench_sfnmf(steps, warmup, F=2049, N=10000, K=1093, Kf=10, Kr=2, seed=0):
    from pyfasst_amd import _lib
    from pyfasst_amd.tools.nmf import _SfNmfContext
    rs = np.random.RandomState(seed)
    SX = rs.gamma(0.7, 1.0, size=(F, N))
    mats = [rs.randn(F, K) ** 2, rs.randn(K, N) ** 2, rs.randn(F, Kf) ** 2, rs.randn(Kf, N) ** 2,
            (1 + rs.randn(F, Kr)) ** 2, (1 + rs.randn(Kr, N)) ** 2]
    mats[0] /= mats[0].sum(axis=0)
    mats[2] /= mats[2].sum(axis=0)
    ptrs = [_lib.dptr(m) for m in mats]
    ctx = _SfNmfContext(F, N, K, Kf, Kr, _lib.default_device())
    _lib.check(_lib.lib.sfnmf_set_data(ctx.ptr, _lib.dptr(SX)), "set_data")
    _lib.check(_lib.lib.sfnmf_set_params(ctx.ptr, *ptrs), "set_params")
    if warmup:
        _lib.check(_lib.lib.sfnmf_run(ctx.ptr, warmup, 1, 1, 1, 1), "run")
    t0 = time.perf_counter()
    _lib.check(_lib.lib.sfnmf_run(ctx.ptr, steps, 1, 1, 1, 1), "run")
    dt = time.perf_counter() - t0
    # per iteration: SF0 formed 3 times, SPHI 3, Sres 2, and two planes per
    # contraction of each of the six updates
    flops = 2.0 * F * N * (K * (3 + 4) + Kf * (3 + 4) + Kr * (2 + 4))
    achieved = flops / (dt / steps) / 1e12
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sfnmf_ref
    cpu_s = None
    if not NO_CPU:
        np.random.seed(seed)
        t1 = time.perf_counter()
        sfnmf_ref.sfnmf_decomp_init(SX, nbComps=K, nbFiltComps=Kf, nbResComps=Kr, niter=1,
                                    Winit=mats[0], Hinit=np.ascontiguousarray(mats[1].T),
                                    WFiltInit=mats[2], HFiltInit=np.ascontiguousarray(mats[3].T))
        cpu_s = time.perf_counter() - t1
    return {"metric": "SFNMF_decomp_init ms per iteration", "value": round(dt / steps * 1e3, 4),
            "unit": "ms/it", "ms_per_step": round(dt / steps * 1e3, 4), "steps": steps,
            "warmup": warmup, "dtype": "f64", "data": "synthetic gamma spectrogram, RandomState(0)",
            "config": {"workload": "source/filter IS-NMF F=%d N=%d K=%d Kf=%d Kr=%d"
                       % (F, N, K, Kf, Kr)},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": FP64_PEAK / 1e12,
                         "unit": "TFLOP/s", "frac": round(achieved * 1e12 / FP64_PEAK, 4),
                         "traffic": None,
                         "scope": "whole iteration, GEMM flops 2FN(7K + 7Kf + 6Kr)"},
            "gemm_tflops_per_s": round(achieved, 2),
            "cpu_baseline": {"value": round(cpu_s * 1e3, 1) if cpu_s else None, "unit": "ms/it",
                             "cores": _blas_threads(), "kind": "port",
                             "sample": "tests/sfnmf_ref.py sfnmf_decomp_init, 1 iteration at the "
                                       "full size"}}


def bench_stereo_nmf(steps, warmup, F=2049, N=10000, R=40, seed=0):
    from pyfasst_amd import _lib
    from pyfasst_amd.SeparateLeadStereo.SIMM.SIMM import _SnmfContext
    from pyfasst_amd.tools.nmf import _NmfContext
    rs = np.random.RandomState(seed)
    SXR = rs.gamma(0.7, 1.0, size=(F, N))
    SXL = rs.gamma(0.7, 1.0, size=(F, N))
    WM = np.abs(rs.randn(F, R))
    HM = np.abs(rs.randn(R, N))
    bR = rs.rand(R)
    dev = _lib.default_device()
    ctx = _SnmfContext(F, N, R, dev)
    _lib.check(_lib.lib.snmf_set_data(ctx.ptr, _lib.dptr(SXR), _lib.dptr(SXL)), "set_data")
    _lib.check(_lib.lib.snmf_set_params(ctx.ptr, _lib.dptr(WM), _lib.dptr(HM), _lib.dptr(bR)),
               "set_params")
    if warmup:
        _lib.check(_lib.lib.snmf_run(ctx.ptr, warmup, 1.0, None), "run")
    t0 = time.perf_counter()
    _lib.check(_lib.lib.snmf_run(ctx.ptr, steps, 1.0, None), "run")
    dt = time.perf_counter() - t0
    errs = np.zeros(3 * steps + 1)
    t0 = time.perf_counter()
    _lib.check(_lib.lib.snmf_run(ctx.ptr, steps, 1.0, _lib.dptr(errs)), "run")
    dt_err = time.perf_counter() - t0
    del ctx
    # three steps, each two hat products and four contractions of 2 F N Rp flops
    Rp = (R + 15) // 16 * 16
    flops = 2.0 * F * N * Rp * 18
    achieved = flops / (dt / steps) / 1e12

    # the yardstick: the IS-NMF engine (one plane, two contractions) in this
    # process, at K = R (its stored-plane GEMM path unless K is a multiple of
    # 16) and at K padded to 16 (its fused path)
    def isnmf(K):
        W = rs.randn(F, K) ** 2
        H = rs.randn(K, N) ** 2
        W /= W.sum(axis=0)
        c = _NmfContext(F, N, K, dev)
        _lib.check(_lib.lib.nmf_set_data(c.ptr, _lib.dptr(SXR)), "set_data")
        _lib.check(_lib.lib.nmf_set_params(c.ptr, _lib.dptr(W), _lib.dptr(H)), "set_params")
        if warmup:
            _lib.check(_lib.lib.nmf_run(c.ptr, warmup, 1, 1), "run")
        t = time.perf_counter()
        _lib.check(_lib.lib.nmf_run(c.ptr, steps, 1, 1), "run")
        return (time.perf_counter() - t) / steps * 1e3
    nmf_ms = {str(K): round(isnmf(K), 4) for K in sorted({R, Rp})}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import stereo_nmf_ref
    cpu_s = None
    if not NO_CPU:
        t1 = time.perf_counter()
        stereo_nmf_ref.iterate(SXR, SXL, WM, HM, np.diag(bR), 1, 1.0)
        cpu_s = time.perf_counter() - t1
    ms = dt / steps * 1e3
    return {"metric": "stereo_NMF ms per iteration", "value": round(ms, 4), "unit": "ms/it",
            "ms_per_step": round(ms, 4), "steps": steps, "warmup": warmup, "dtype": "f64",
            "ms_per_step_with_error_vector": round(dt_err / steps * 1e3, 4),
            "data": "synthetic gamma spectrograms, RandomState(0)",
            "config": {"workload": "stereo IS-NMF F=%d N=%d R=%d" % (F, N, R)},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": FP64_PEAK / 1e12,
                         "unit": "TFLOP/s", "frac": round(achieved * 1e12 / FP64_PEAK, 4),
                         "traffic": None, "scope": "whole iteration, MFMA flops 36 F N Rp"},
            "isnmf_ms_per_step": nmf_ms,
            "ratio_to_isnmf": {k: round(ms / v, 3) for k, v in nmf_ms.items()},
            "cpu_baseline": {"value": round(cpu_s * 1e3, 1) if cpu_s else None, "unit": "ms/it",
                             "cores": _blas_threads(), "kind": "port",
                             "sample": "tests/stereo_nmf_ref.py iterate, 1 iteration (and the "
                                       "initial model and error) at the full size"}}


def bench_sigtools(steps, warmup, F=2049, N=10000, seed=0):
    from pyfasst_amd.tools import signalTools as st
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sigtools_ref as S
    rs = np.random.RandomState(seed)
    X0 = rs.randn(F, N) + 1j * rs.randn(F, N)
    X1 = rs.randn(F, N) + 1j * rs.randn(F, N) + 0.5 * X0
    TF = rs.gamma(0.7, 1.0, size=(F, N))
    rows = rs.randn(3, N)
    nb, length = 20, 10
    L = N - nb + 1

    def timed(fn, ref):
        for _ in range(warmup):
            fn()
        dev, wall = [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            wall.append(time.perf_counter() - t0)
            dev.append(st.last_ms())
        cpu_s = None
        if not NO_CPU:
            t1 = time.perf_counter()
            ref()
            cpu_s = time.perf_counter() - t1
        return float(np.median(dev)), float(np.median(wall)) * 1e3, cpu_s

    def case(name, fn, ref, nbytes, what):
        dev_ms, wall_ms, cpu_s = timed(fn, ref)
        gbs = nbytes / (dev_ms * 1e-3) / 1e9
        return {"case": name, "device_ms": round(dev_ms, 4), "host_inclusive_ms": round(wall_ms, 2),
                "hbm_bytes": int(nbytes), "hbm_gb_per_s": round(gbs, 1),
                "frac_of_measured_copy_6290": round(gbs / 6290., 4), "bytes_counted": what,
                "cpu_restatement_ms": round(cpu_s * 1e3, 1) if cpu_s else None}

    kw = dict(samplingrate=44100, fouriersize=2 * (F - 1))
    ptr, _ = st.harmonic_bins(np.arange(F) * 44100 / np.double(2 * (F - 1)), st.f0_table(), 20, 0.5)
    cases = [
        case("prinComp2D F=%d N=%d neighborNb=%d" % (F, N, nb),
             lambda: st.prinComp2D(X0, X1, neighborNb=nb), lambda: S.prin_comp_2d(X0, X1, nb),
             2 * 16 * F * N + (2 * 8 + 4 * 16) * F * L, "both planes read once, six planes written"),
        case("harmonicSum F=%d T=%d default grid (%d F0s, %d selected bins)"
             % (F, N, st.f0_table().size, ptr[-1]),
             lambda: st.harmonicSum(TF, **kw), lambda: S.f0_detection(TF, **kw),
             2 * 8 * F * N + 8 * st.f0_table().size * N,
             "TF read twice (column sums, maxima), hs written; re-reads of bins shared by "
             "several F0s are cache traffic and not counted"),
        case("medianFilter R=3 N=%d length=%d" % (N, length),
             lambda: st.median_rows(rows, length),
             lambda: [S.median_filter(r, length) for r in rows],
             2 * 8 * 3 * N, "rows read and written once"),
    ]
    return {"metric": "signalTools device ms (prinComp2D)", "value": cases[0]["device_ms"],
            "unit": "ms", "ms_per_step": cases[0]["device_ms"], "steps": steps, "warmup": warmup,
            "dtype": "f64", "data": "synthetic, RandomState(0)",
            "config": {"workload": "signalTools: prinComp2D, harmonicSum, medianFilter"},
            "cases": cases,
            "roofline": {"bound": "hbm", "achieved": cases[0]["hbm_gb_per_s"], "peak": 6290.,
                         "unit": "GB/s", "frac": cases[0]["frac_of_measured_copy_6290"],
                         "traffic": cases[0]["hbm_bytes"], "scope": "k_pca2d, device events"},
            "cpu_baseline": {"value": cases[0]["cpu_restatement_ms"], "unit": "ms",
                             "cores": _blas_threads(), "kind": "port",
                             "sample": "tests/sigtools_ref.py at the full size, once per case "
                                       "(cases[*].cpu_restatement_ms)"}}


def bench_demix(steps, warmup, fs=44100, wlen=2048, hop=1024, frames=5000, neighbors=20, seed=0):
    """DEMIX (demixTF.py) on about two minutes of synthetic stereo: three band
    noises with pans and integer delays plus white noise, 5000 hops of 1024
    samples at 44.1 kHz (5.12 M samples, under the two-minute crop): F = 1025,
    N = 5002 frames, L = 4983 windows with neighbors = 20.  Device times are
    HIP events around the kernels (DEMIX.features_ms, round_pass_ms); the
    restatement (tests/demix_ref.py, direct PCA sums) runs once on this host."""
    import tempfile
    import warnings
    import scipy.io.wavfile as wf
    import pyfasst_amd.demixTF as dm
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import demix_ref as D
    n = frames * hop
    x = D.live_mixture(n, seed, fs=fs)
    samples = np.round(x / np.abs(x).max() * 30000).astype(np.int16)
    kw = dict(nsources=3, wlen=wlen, hopsize=hop, neighbors=neighbors)
    runs = []
    with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
        warnings.simplefilter('ignore')
        wav = os.path.join(tmp, "demix.wav")
        wf.write(wav, fs, samples)
        for it in range(warmup + steps):
            d = dm.DEMIX(wav, **kw)
            t0 = time.perf_counter()
            d.comp_clusters()
            t1 = time.perf_counter()
            passes = np.array(d.round_pass_ms)
            full = ~np.isnan([c.delta for c in d.clusterCentroids])
            npts = d._F * d._L
            shape = (d._F, d._L)
            d.refine_clusters()
            t2 = time.perf_counter()
            if it >= warmup:
                runs.append(dict(features=d.features_ms, round=float(np.mean(d.round_ms)),
                                 argmax=float(np.mean(passes[:, 0])),
                                 theta=float(np.mean(passes[:, 1])),
                                 delta=float(np.mean(passes[full, 2])) if full.any() else None,
                                 rounds=len(d.round_ms), rounds_with_delta=int(full.sum()),
                                 comp=(t1 - t0) * 1e3, refine=(t2 - t1) * 1e3))
            result = [(float(c.theta), float(c.delta)) for c in d.clusterCentroids]
            del d
    med = lambda k: float(np.median([r[k] for r in runs if r[k] is not None]))
    cpu = None
    if not NO_CPU:
        print("restatement: comp_clusters ...", file=sys.stderr, flush=True)
        r = D.RefDEMIX(D.read_scaled(samples), fs, pca='direct', **kw)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t0 = time.perf_counter()
            r.comp_clusters()
            t1 = time.perf_counter()
            print("restatement: refine_clusters ...", file=sys.stderr, flush=True)
            r.refine_clusters()
            t2 = time.perf_counter()
        cpu = {"comp_clusters_ms": round((t1 - t0) * 1e3, 1),
               "refine_clusters_ms": round((t2 - t1) * 1e3, 1), "rounds": len(r.rounds),
               "centroids": [(float(c.theta), float(c.delta)) for c in r.clusterCentroids]}
    theta_bytes, delta_bytes = 26 * npts, 35 * npts
    gbs = lambda b, ms: round(b / (ms * 1e-3) / 1e9, 1)
    th, de = med('theta'), med('delta')
    return {"metric": "DEMIX device ms per clustering round", "value": round(med('round'), 4),
            "unit": "ms", "ms_per_step": round(med('round'), 4), "steps": steps, "warmup": warmup,
            "dtype": "f64", "data": "synthetic, demix_ref.live_mixture(%d, %d, fs=%d)" % (n, seed, fs),
            "config": {"workload": "DEMIX F=%d N=%d L=%d neighbors=%d nsources=3 maxclusters=100"
                                   % (shape[0], frames + 2, shape[1], neighbors)},
            "features_device_ms": round(med('features'), 4),
            "round_device_ms": round(med('round'), 4),
            "argmax_device_ms": round(med('argmax'), 4),
            "theta_pass_device_ms": round(th, 4), "delta_pass_device_ms": round(de, 4),
            "rounds": runs[-1]['rounds'], "rounds_with_delta": runs[-1]['rounds_with_delta'],
            "comp_clusters_host_inclusive_ms": round(med('comp'), 1),
            "refine_clusters_host_inclusive_ms": round(med('refine'), 1),
            "centroids": result,
            "passes": [
                {"pass": "k_theta_pass", "hbm_bytes": theta_bytes, "hbm_gb_per_s": gbs(theta_bytes, th),
                 "frac_of_measured_copy_6290": round(gbs(theta_bytes, th) / 6290., 4),
                 "bytes_counted": "theta, phi, var and the subset byte read, the candidate byte "
                                  "written (26 B per point)"},
                {"pass": "k_delta_pass", "hbm_bytes": delta_bytes, "hbm_gb_per_s": gbs(delta_bytes, de),
                 "frac_of_measured_copy_6290": round(gbs(delta_bytes, de) / 6290., 4),
                 "bytes_counted": "four planes and the subset byte read, the mask byte and the "
                                  "subset byte written (35 B per point); rounds with a delta"}],
            "roofline": {"bound": "hbm", "achieved": gbs(delta_bytes, de), "peak": 6290.,
                         "unit": "GB/s", "frac": round(gbs(delta_bytes, de) / 6290., 4),
                         "traffic": delta_bytes, "scope": "k_delta_pass, device events"},
            "cpu_baseline": {"value": cpu["comp_clusters_ms"] if cpu else None, "unit": "ms",
                             "cores": _blas_threads(), "kind": "port",
                             "sample": "tests/demix_ref.py comp_clusters() then refine_clusters() "
                                       "on the same samples, once", "detail": cpu}}


def bench_filter(steps, warmup, M=2, L=5120000, wlen=4096, hop=512, seed=0):
    """filter_stft at the C3 clip (2 channels, 5.12 M samples, wlen = nfft =
    4096, hop 512: 10000 frames), time-invariant and time-varying W, against
    the route it replaces: stft() per channel, a host product, istft() per
    channel."""
    import ctypes
    from pyfasst_amd import _lib
    from pyfasst_amd.tftransforms.stft import filter_stft, istft, stft
    rs = np.random.RandomState(seed)
    F, N = wlen // 2 + 1, -(-L // hop)
    x = rs.randn(L, M)
    sw = np.sin(np.pi * np.arange(wlen) / (1.0 * wlen))
    aw = np.hanning(wlen) + 0.1
    kw = dict(analysisWindow=aw, synthWindow=sw, hopsize=float(hop), nfft=float(wlen))
    rows = (N - 1) * hop + wlen - wlen // 2

    _lib.lib.fasst_filter_set_timing(1)

    def last_ms():
        tot, tr = ctypes.c_double(0), ctypes.c_double(0)
        _lib.lib.fasst_filter_last_ms(ctypes.byref(tot), ctypes.byref(tr))
        return tot.value, tr.value

    def replaced(W):
        X = np.array([stft(x[:, c], window=aw, hopsize=hop, nfft=wlen)[0] for c in range(M)])
        Wn = W[..., :X.shape[2]] if W.ndim == 4 else W[..., None]
        Y = np.einsum('ocfn,cfn->ofn', Wn, X)
        return np.stack([istft(Y[c], window=sw, analysisWindow=aw, hopsize=hop, nfft=wlen)
                         for c in range(M)], axis=1)

    cases = []
    for tv in (False, True):
        # the replaced route frames with ceil(L/hop) + 2 frames: W covers them
        shape = (M, M, F) + ((N + 2,) if tv else ())
        W = np.empty(shape, dtype=np.complex128)
        W.real = rs.randn(*shape)
        W.imag = rs.randn(*shape)
        for _ in range(warmup):
            filter_stft(x, W, **kw)
        dev, tr, wall = [], [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            filter_stft(x, W, **kw)
            wall.append(time.perf_counter() - t0)
            a, b = last_ms()
            dev.append(a)
            tr.append(b)
        t1 = time.perf_counter()
        replaced(W)
        old_s = time.perf_counter() - t1
        t1 = time.perf_counter()
        replaced(W)
        old_s = min(old_s, time.perf_counter() - t1)
        w_bytes = 16 * W.size
        nbytes = (w_bytes * (3 if tv else 1) + 2 * 8 * M * N * wlen + 8 * M * L + 8 * M * rows)
        dev_ms = float(np.median(dev))
        gbs = nbytes / (dev_ms * 1e-3) / 1e9
        cases.append({"case": "filter_stft M=%d L=%d wlen=nfft=%d hop=%d (%d frames), W %s"
                              % (M, L, wlen, hop, N, "time-varying" if tv else "time-invariant"),
                      "device_ms": round(dev_ms, 3),
                      "of_which_w_transpose_ms": round(float(np.median(tr)), 3),
                      "host_inclusive_ms": round(float(np.median(wall)) * 1e3, 1),
                      "replaced_route_host_inclusive_ms": round(old_s * 1e3, 1),
                      "w_bytes": int(w_bytes), "hbm_bytes": int(nbytes),
                      "hbm_gb_per_s": round(gbs, 1),
                      "frac_of_measured_copy_6290": round(gbs / 6290., 4),
                      "bytes_counted": "W read once%s, frames written and read (2*8*M*N*wlen), "
                                       "data read, output written"
                                       % (" plus the transpose's read and write" if tv else "")})
        del W
    return {"metric": "filter_stft device ms (time-invariant W)", "value": cases[0]["device_ms"],
            "unit": "ms", "ms_per_step": cases[0]["device_ms"], "steps": steps, "warmup": warmup,
            "dtype": "f64", "data": "synthetic, RandomState(0)",
            "config": {"workload": "filter_stft, C3 clip", "M": M, "L": L, "wlen": wlen, "hop": hop},
            "cases": cases,
            "roofline": {"bound": "hbm", "achieved": cases[0]["hbm_gb_per_s"], "peak": 6290.,
                         "unit": "GB/s", "frac": cases[0]["frac_of_measured_copy_6290"],
                         "traffic": cases[0]["hbm_bytes"],
                         "scope": "transpose + k_filter_frames + k_ola_ch, device events"},
            "cpu_baseline": {"value": cases[0]["replaced_route_host_inclusive_ms"], "unit": "ms",
                             "cores": _blas_threads(), "kind": "replaced route",
                             "sample": "stft() per channel on the GPU, NumPy product on the host, "
                                       "istft() per channel on the GPU, best of two"}}


def bench_dirdiag(steps, warmup, F=2049, T=10000, ntheta=512, seed=0):
    """dir_diag_stereo at the headline size: the resident route (the model's
    planes, nothing but the diagram crosses) against the host-array route
    (Cx uploaded as an observation first), device time per kernel."""
    from pyfasst_amd.engine import Engine
    from pyfasst_amd.spatial import steering_vectors as sv
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spatial_pkg_ref as S
    rs = np.random.RandomState(seed)
    X = rs.randn(2, F, T) + 1j * rs.randn(2, F, T)
    X[1] += 0.5 * X[0]
    Cx = np.array([X[0] * np.conjugate(X[0]), X[0] * np.conjugate(X[1]), X[1] * np.conjugate(X[1])])
    del X
    kw = dict(nft=2 * (F - 1), ntheta=ntheta, samplerate=44100, distanceInterMic=0.3)
    eng = Engine(F, T)
    eng.set_cx(Cx)

    def timed(fn):
        for _ in range(warmup):
            fn()
        wall, ms = [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            wall.append(time.perf_counter() - t0)
            ms.append(sv.last_ms())
        return float(np.median(wall)) * 1e3, {k: float(np.median([m[k] for m in ms])) for k in ms[0]}

    res_ms, kern = timed(lambda: eng.dir_diag(ntheta, 0.3, kw['nft'], 44100))
    host_ms, _ = timed(lambda: sv.dir_diag_stereo(Cx, **kw))
    d = eng.dir_diag(ntheta, 0.3, kw['nft'], 44100)[0]
    cpu_s = err = None
    if not NO_CPU:
        t1 = time.perf_counter()
        ref = S.dir_diag_stereo(Cx, **kw)[0]
        cpu_s = time.perf_counter() - t1
        err = S.rel_max(d, ref)
    nbytes = 4 * 8 * F * T
    gbs = nbytes / (kern['k_cx_tmean'] * 1e-3) / 1e9
    return {"metric": "dir_diag_stereo resident route, host-inclusive ms", "value": round(res_ms, 3),
            "unit": "ms", "ms_per_step": round(res_ms, 3), "steps": steps, "warmup": warmup,
            "dtype": "f64", "data": "synthetic, RandomState(0)",
            "config": {"workload": "dir_diag_stereo F=%d T=%d ntheta=%d" % (F, T, ntheta)},
            "device_ms": {"k_cx_tmean": round(kern['k_cx_tmean'], 4),
                          "k_capon_diagram": round(kern['k_capon_diagram'], 4)},
            "resident_route_host_inclusive_ms": round(res_ms, 3),
            "host_array_route_host_inclusive_ms": round(host_ms, 2),
            "rel_err_vs_restatement": err,
            "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": COPY_GBS, "unit": "GB/s",
                         "frac": round(gbs / COPY_GBS, 4), "traffic": int(nbytes),
                         "scope": "k_cx_tmean (partial and combine launch), device events; the "
                                  "four planes read once, against the device copy rate of "
                                  "profiles/sigtools_bench.jsonl"},
            "cpu_baseline": {"value": round(cpu_s * 1e3, 1) if cpu_s else None, "unit": "ms",
                             "cores": _blas_threads(), "kind": "port",
                             "sample": "tests/spatial_pkg_ref.py dir_diag_stereo at the full size, "
                                       "once"}}


def bench_nsgt(steps, warmup, fs=44100, Ls=4410000, bins=48, fmin=27.5, fmax=18000, seed=0):
    """CQ_NSGT of 100 s of audio, one and two channels: device time of forward
    and backward (plan resident; events around the kernels), host-inclusive
    time from NumPy arrays, and the NumPy restatement on this box's cores; the
    runs of the two channel counts alternate."""
    import warnings
    from pyfasst_amd.tftransforms.nsgt import CQ_NSGT, _device
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nsgt_ref as NR
    rs = np.random.RandomState(seed)
    x2 = rs.randn(2, Ls)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        tr = {1: CQ_NSGT(fmin, fmax, bins, fs, Ls, real=True),
              2: CQ_NSGT(fmin, fmax, bins, fs, Ls, real=True, multichannel=True)}
        plan_host_s = (time.perf_counter() - t0) / 2
    sig = {1: x2[0], 2: x2}
    _device.set_timing(True)
    t0 = time.perf_counter()
    coef = {n: tr[n].forward(sig[n]) for n in (1, 2)}    # builds the device plans
    plan_dev_s = (time.perf_counter() - t0) / 2
    acc = {(n, d): {"dev": [], "fft": [], "wall": []} for n in (1, 2) for d in "fb"}
    for it in range(warmup + steps):
        for n in (1, 2):
            for d in "fb":
                t0 = time.perf_counter()
                if d == "f":
                    tr[n].forward(sig[n])
                else:
                    y = tr[n].backward(coef[n])
                wall = time.perf_counter() - t0
                if it >= warmup:
                    a = acc[(n, d)]
                    tot, part = _device.last_ms()
                    a["dev"].append(tot)
                    a["fft"].append(part)
                    a["wall"].append(wall * 1e3)
    err = float(np.max(np.abs(np.asarray(y) - x2)) / np.max(np.abs(x2)))
    p = tr[1].plan
    sh = 1 << int(np.ceil(np.log2(2 * Ls - 1)))
    # the convolution's 2 FFTs of P points (the chirp's spectrum, the third, is
    # tabulated in the plan), 2 passes each, read + write, 16 B
    fft_bytes = 2 * 2 * 2 * 16 * sh
    cases = []
    for n in (1, 2):
        for d, nm in (("f", "forward"), ("b", "backward")):
            a = acc[(n, d)]
            dev, fft = float(np.median(a["dev"])), float(np.median(a["fft"]))
            gbs = n * fft_bytes / (fft * 1e-3) / 1e9
            cases.append({"case": "%s, %d channel%s" % (nm, n, "s" if n > 1 else ""),
                          "device_ms": round(dev, 3), "signal_fft_ms": round(fft, 3),
                          "band_stage_ms": round(dev - fft, 3),
                          "host_inclusive_ms": round(float(np.median(a["wall"])), 1),
                          "signal_fft_gb_per_s": round(gbs, 1),
                          "signal_fft_frac_of_copy": round(gbs / COPY_GBS, 4)})
    cpu = None
    if not NO_CPU:
        f, q = NR.oct_scale(fmin, fmax, bins)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rp = NR.Plan(f, q, fs, Ls)
        t0 = time.perf_counter()
        rc = rp.forward(x2[0])
        cf = time.perf_counter() - t0
        t0 = time.perf_counter()
        rp.backward(rc)
        cb = time.perf_counter() - t0
        cpu = {"forward_ms": round(cf * 1e3, 1), "backward_ms": round(cb * 1e3, 1)}
    return {"metric": "CQ_NSGT forward device ms, 1 channel", "value": cases[0]["device_ms"],
            "unit": "ms", "ms_per_step": cases[0]["device_ms"], "steps": steps, "warmup": warmup,
            "dtype": "f64", "data": "synthetic, RandomState(0)",
            "config": {"workload": "CQ_NSGT fmin=%g fmax=%g bins=%d fs=%d Ls=%d real" % (
                fmin, fmax, bins, fs, Ls), "bands": len(tr[1].g), "coef_len": int(p.coef_len),
                "bluestein_P": sh},
            "cases": cases, "round_trip_rel_err": err,
            "plan_host_s": round(plan_host_s, 2), "plan_device_s": round(plan_dev_s, 2),
            "roofline": {"bound": "hbm", "achieved": cases[0]["signal_fft_gb_per_s"],
                         "peak": COPY_GBS, "unit": "GB/s",
                         "frac": cases[0]["signal_fft_frac_of_copy"], "traffic": int(fft_bytes),
                         "scope": "the Ls-point Bluestein FFT: 2 FFTs of P points per call (the "
                                  "third, of the chirp, is tabulated) x 2 passes x (read + "
                                  "write) x 16 B, device events"},
            "cpu_baseline": {"value": cpu["forward_ms"] if cpu else None, "unit": "ms",
                             "cores": _blas_threads(), "kind": "port", "detail": cpu,
                             "sample": "tests/nsgt_ref.py forward / backward of one channel "
                                       "(numpy.fft), once, planning excluded"}}


def bench_slicq(steps, warmup, fs=44100, L=4410000, bins=48, fmin=27.5, fmax=18000, sl_len=65536,
                tr_area=4096, seed=0):
    """CQ_NSGT_sliced of 100 s of audio, one and two channels: device time of
    forward and backward (plan resident; events around the kernels of every
    call, summed over the calls of one transform), host-inclusive time of the
    generators from and to NumPy arrays, the round trip; alongside, the
    whole-signal CQ_NSGT of the same signal and the NumPy restatement of the
    sliced transform on this box's cores."""
    import warnings
    from pyfasst_amd.tftransforms.nsgt import CQ_NSGT, _device
    from pyfasst_amd.tftransforms.slicq import CQ_NSGT_sliced
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nsgt_ref as NR
    import slicq_ref as SR
    rs = np.random.RandomState(seed)
    x2 = rs.randn(2, L)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr = {1: CQ_NSGT_sliced(fmin, fmax, bins, sl_len, tr_area, fs, real=True),
              2: CQ_NSGT_sliced(fmin, fmax, bins, sl_len, tr_area, fs, real=True,
                                multichannel=True)}
        whole = CQ_NSGT(fmin, fmax, bins, fs, L, real=True)
    sig = {1: x2[0], 2: x2}
    _device.set_timing(True)
    coef = {n: list(tr[n].forward((sig[n],))) for n in (1, 2)}    # builds the device plans
    packed = {1: np.array([[np.concatenate(c)] for c in coef[1]]),
              2: np.array([[np.concatenate(ch) for ch in it] for it in coef[2]])}
    nsl = len(coef[1])

    def device_pass(n, d):
        """One transform through the plan's batched calls: (total, slicing + FFT share) ms."""
        t, p, tot, part = tr[n], tr[n].plan, 0.0, 0.0
        if d == "f":
            for first, run in t._runs((sig[n],)):
                p.slices_forward(run, first)
                a, b = _device.last_ms()
                tot, part = tot + a, part + b
        else:
            per = t._per_call(n)
            carry = np.zeros((n, 2 * t.hhop))
            for first in range(0, nsl, per):
                p.slices_backward(packed[n][first:first + per], carry, first)
                a, b = _device.last_ms()
                tot, part = tot + a, part + b
        return tot, part

    acc = {(n, d): {"dev": [], "fft": [], "wall": []} for n in (1, 2) for d in "fb"}
    for it in range(warmup + steps):
        for n in (1, 2):
            for d in "fb":
                tot, part = device_pass(n, d)
                t0 = time.perf_counter()
                if d == "f":
                    list(tr[n].forward((sig[n],)))
                else:
                    y = np.concatenate(list(tr[n].backward(coef[n])), axis=-1)
                wall = time.perf_counter() - t0
                if it >= warmup:
                    a = acc[(n, d)]
                    a["dev"].append(tot)
                    a["fft"].append(part)
                    a["wall"].append(wall * 1e3)
    err = float(np.max(np.abs(y[:, :L] - x2)) / np.max(np.abs(x2)))
    p = tr[1].plan
    cases = []
    for n in (1, 2):
        # slicing (stream read once, slices written) and the sl_len-point
        # four-step FFT (2 passes, read + write, 16 B; its first read is the 8 B slices)
        fwd_bytes = n * (8 * (2 * nsl + 2) * (sl_len // 4) + nsl * sl_len * (8 + 8 + 16 + 16 + 16))
        # the nn-point inverse FFT (2 passes, the last write 8 B) and the unslicing
        bwd_bytes = n * (nsl * sl_len * (16 + 16 + 16 + 8 + 8) + 8 * 2 * nsl * (sl_len // 4))
        for d, nm, nbytes in (("f", "forward", fwd_bytes), ("b", "backward", bwd_bytes)):
            a = acc[(n, d)]
            dev, fft = float(np.median(a["dev"])), float(np.median(a["fft"]))
            # forward: the share is slicing + slice FFT; backward: the inverse FFT + unslicing
            gbs = nbytes / (fft * 1e-3) / 1e9
            cases.append({"case": "%s, %d channel%s" % (nm, n, "s" if n > 1 else ""),
                          "device_ms": round(dev, 3), "slice_fft_ms": round(fft, 3),
                          "band_stage_ms": round(dev - fft, 3),
                          "host_inclusive_ms": round(float(np.median(a["wall"])), 1),
                          "slice_fft_gb_per_s": round(gbs, 1),
                          "slice_fft_frac_of_copy": round(gbs / COPY_GBS, 4)})
    # the whole-signal transform of the same signal, same session
    wc = whole.forward(x2[0])
    wacc = {"f": [], "b": []}
    for it in range(warmup + steps):
        whole.forward(x2[0])
        wacc["f"].append(_device.last_ms()[0])
        whole.backward(wc)
        wacc["b"].append(_device.last_ms()[0])
    whole_ms = {"forward_ms": round(float(np.median(wacc["f"][warmup:])), 3),
                "backward_ms": round(float(np.median(wacc["b"][warmup:])), 3),
                "coef_len": int(whole.plan.coef_len)}
    cpu = None
    if not NO_CPU:
        f, q = NR.oct_scale(fmin, fmax, bins)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rp = SR.SlicedPlan(f, q, fs, sl_len, tr_area, real=True)
        t0 = time.perf_counter()
        rc = rp.forward_stream(x2[0])
        cf = time.perf_counter() - t0
        t0 = time.perf_counter()
        rp.backward_stream(rc)
        cb = time.perf_counter() - t0
        cpu = {"forward_ms": round(cf * 1e3, 1), "backward_ms": round(cb * 1e3, 1)}
    return {"metric": "CQ_NSGT_sliced forward device ms, 1 channel", "value": cases[0]["device_ms"],
            "unit": "ms", "ms_per_step": cases[0]["device_ms"], "steps": steps, "warmup": warmup,
            "dtype": "f64", "data": "synthetic, RandomState(0)",
            "config": {"workload": "CQ_NSGT_sliced fmin=%g fmax=%g bins=%d sl_len=%d tr_area=%d "
                                   "fs=%d L=%d real" % (fmin, fmax, bins, sl_len, tr_area, fs, L),
                       "bands": len(tr[1].g), "coef_len": int(p.coef_len), "slices": nsl,
                       "slices_per_call": tr[1].slices_per_call},
            "cases": cases, "round_trip_rel_err": err, "whole_signal_cq_nsgt": whole_ms,
            "roofline": {"bound": "hbm", "achieved": cases[0]["slice_fft_gb_per_s"],
                         "peak": COPY_GBS, "unit": "GB/s",
                         "frac": cases[0]["slice_fft_frac_of_copy"],
                         "scope": "forward: k_slice and the sl_len-point four-step FFT of every "
                                  "slice; backward: the inverse FFT and k_unslice; minimal "
                                  "traffic over the device events of that share"},
            "cpu_baseline": {"value": cpu["forward_ms"] if cpu else None, "unit": "ms",
                             "cores": _blas_threads(), "kind": "port", "detail": cpu,
                             "sample": "tests/slicq_ref.py forward_stream / backward_stream of "
                                       "one channel (numpy.fft), once, planning excluded"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("simm", "nmf", "cqt", "viterbi", "wf0", "separate",
                                           "nnls", "spatial", "hmm", "sf", "sfnmf", "sigtools",
                                           "separate_cqt", "filter", "stereo_nmf", "demix",
                                           "wf0_chirped", "dirdiag", "nsgt", "slicq"),
                    required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="skip the CPU baseline (profiling passes)")
    ap.add_argument("--sparsity", type=int, default=0,
                    help="sf: median length L of the sparsity reweighting (0: off)")
    a = ap.parse_args()
    global NO_CPU
    NO_CPU = a.no_cpu_baseline
    fn = {"simm": bench_simm, "nmf": bench_nmf, "cqt": bench_cqt, "viterbi": bench_viterbi,
          "wf0": bench_wf0, "separate": bench_separate, "nnls": bench_nnls,
          "spatial": bench_spatial, "hmm": bench_hmm, "sf": bench_sf,
          "sfnmf": bench_sfnmf, "sigtools": bench_sigtools,
          "separate_cqt": bench_separate_cqt, "filter": bench_filter,
          "stereo_nmf": bench_stereo_nmf, "demix": bench_demix,
          "wf0_chirped": bench_wf0_chirped, "dirdiag": bench_dirdiag,
          "nsgt": bench_nsgt, "slicq": bench_slicq}[a.workload]
    out = fn(a.steps, a.warmup, sparsity=a.sparsity) if a.workload == "sf" else \
        fn(a.steps, a.warmup)
    if NO_CPU:
        out["cpu_baseline"] = None   # not measured (the sample above timed nothing)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
