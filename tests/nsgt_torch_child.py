"""Child process of tests/test_gpu_nsgt.py: the torch-tensor route of NSGT
forward / backward.  It runs in a process of its own because torch must have
initialised the GPU before the library's first device call.  Prints one JSON
line: per case, what was checked.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

CASES = ["prime", "even", "wideband", "stereo"]


def main():
    dev = torch.device('cuda', 0)
    torch.zeros(1, device=dev)                       # torch initialises the GPU first
    import nsgt_ref as NR
    from pyfasst_amd.tftransforms.nsgt import CQ_NSGT
    out = {}
    for name in CASES:
        c = NR.CASES[name]
        multi = "nch" in c
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = CQ_NSGT(c["fmin"], c["fmax"], c["bins"], c["fs"], c["Ls"], real=c["real"],
                        multichannel=multi)
        x = NR.signal(name)
        host_c = t.forward(x)                        # the NumPy route
        host_y = np.asarray(t.backward(host_c))
        flat = (np.array([np.concatenate(ch) for ch in host_c]) if multi
                else np.concatenate(host_c))
        tx = torch.as_tensor(x, device=dev)
        tc, off = t.forward(tx)
        ty = t.backward((tc, off))
        r = {"tensor_out": bool(torch.is_tensor(tc) and tc.device == dev
                                and tc.dtype == torch.complex128 and torch.is_tensor(ty)
                                and ty.device == dev),
             "offsets_ok": bool(np.array_equal(np.diff(off), [len(b) for b in
                                                              (host_c[0] if multi else host_c)])
                                and tc.shape[-1] == off[-1]),
             "forward_bit_equal": bool(np.array_equal(tc.cpu().numpy(), flat)),
             "backward_bit_equal": bool(np.array_equal(ty.cpu().numpy(), host_y))}
        # a producer's pending work on the current stream is waited for
        y2 = t.backward(t.forward(tx * 2.0)[0])
        r["scaled"] = float(np.max(np.abs(y2.cpu().numpy() - 2.0 * x)) / np.max(np.abs(x)))
        out[name] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
