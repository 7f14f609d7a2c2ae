"""Child process of tests/test_gpu_filter_stft.py: the torch-tensor route of
filter_stft / filter_conv_stft.  It runs in a process of its own because
torch must have initialised the GPU before the library's first device call
(the two bring their own HIP runtimes; in the other order torch finds no
device).  Prints one JSON line: per case, what was checked.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

CASES = ["base_m2", "m5_surplus", "short_m3", "m4_tv_real", "conv_m3_col", "conv_m1", "lds_4096"]


def main():
    dev = torch.device('cuda', 0)
    torch.zeros(1, device=dev)                       # torch initialises the GPU first
    import filter_stft_ref as FR
    from pyfasst_amd.tftransforms.stft import filter_conv_stft, filter_stft
    out = {}
    for name in CASES:
        c = FR.CASES[name]
        data, W, aw, sw = FR.draw(name)
        fn = filter_stft if c['fn'] == 'stft' else filter_conv_stft
        kw = dict(analysisWindow=aw, synthWindow=sw, hopsize=float(c['hop']), nfft=float(c['nfft']))
        host = fn(data, W, **kw)                     # the NumPy route
        td, tW = torch.as_tensor(data, device=dev), torch.as_tensor(W, device=dev)
        y = fn(td, tW, **kw)
        r = {"tensor_out": bool(torch.is_tensor(y) and y.device == dev and y.dtype == torch.float64),
             "bit_equal": bool(np.array_equal(y.cpu().numpy(), host))}
        tv = W.ndim == (4 if c['fn'] == 'stft' else 3)
        if tv:
            tWf = torch.movedim(tW.to(torch.complex128), -1, -2).contiguous()      # [.., N, F]
            yf = fn(td, tWf, w_frame_major=True, **kw)
            r["frame_major_bit_equal"] = bool(np.array_equal(yf.cpu().numpy(), host))
        else:
            try:
                fn(td, tW, w_frame_major=True, **kw)
                r["frame_major_refused"] = False
            except ValueError:
                r["frame_major_refused"] = True
        ym = fn(data, tW, **kw)                      # NumPy data, tensor W: W's device
        r["mixed_bit_equal"] = bool(torch.is_tensor(ym) and np.array_equal(ym.cpu().numpy(), host))
        # a producer's pending work on the current stream is waited for
        y2 = fn(td * 2.0, tW, **kw)
        r["scaled"] = float(np.max(np.abs(y2.cpu().numpy() - 2.0 * host)) / np.max(np.abs(host)))
        out[name] = r
    errs = {}
    x = torch.zeros(200, 2, dtype=torch.float64, device=dev)
    kw = dict(synthWindow=FR.sinebell(64), hopsize=16.0, nfft=64.0)
    for key, exc, call in (
            ("channels", AttributeError, lambda: filter_stft(x, torch.zeros(3, 3, 33, device=dev), **kw)),
            ("bins", AttributeError, lambda: filter_stft(x, torch.zeros(2, 2, 65, device=dev), **kw)),
            ("ndim", NotImplementedError,
             lambda: filter_stft(x, torch.zeros(2, 2, 33, 13, 1, device=dev), **kw)),
            ("frames", IndexError, lambda: filter_stft(x, torch.zeros(2, 2, 33, 12, device=dev), **kw)),
            ("single", AttributeError, lambda: filter_conv_stft(x, torch.zeros(2, 33, device=dev), **kw)),
            ("conv_ndim", ValueError,
             lambda: filter_conv_stft(x[:, 0], torch.zeros(2, 33, 13, 1, device=dev), **kw)),
            ("cpu_tensor", ValueError, lambda: filter_stft(x.cpu(), torch.zeros(2, 2, 33), **kw))):
        try:
            call()
            errs[key] = "no exception"
        except exc:
            errs[key] = "ok"
        except Exception as e:          # noqa: BLE001  (reported to the parent)
            errs[key] = "%s: %s" % (type(e).__name__, e)
    print(json.dumps({"cases": out, "errors": errs}), flush=True)


if __name__ == "__main__":
    main()
